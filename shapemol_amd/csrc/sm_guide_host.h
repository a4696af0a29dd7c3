// Host side of the guidance of a chain's predicted x0: which kind a chain uses (chain_guide), the launches of every kind
// (enqueue_guidance), their device data (setters) and the stand-alone entry points of the C ABI.  Included by
// shapemol_hip.hip behind shapemol_ctx and the LAUNCH / SMK macros.
#pragma once

namespace {

// The guidance of the chains to come: the reference's if / elif in sample_diffusion -- mesh (one for the batch, or one per group
// of molecules), else the point cloud (likewise: the setters keep at most one of each two), else classifier-free guidance.
// Groups without any mesh / cloud guide nothing (and leave the next kind its turn).  The only place that spells this out.
Guide chain_guide(const shapemol_ctx *c) {
    if (c->m_nfaces > 0) return Guide::Mesh;
    if (c->mg_groups > 0 && c->mg_nfaces > 0) return Guide::MeshGroups;
    if (c->g_points > 0) return Guide::Cloud;
    if (c->gg_groups > 0 && c->gg_points > 0) return Guide::Groups;
    return c->cfg_w != 0.0 ? Guide::Cfg : Guide::None;
}

// launch shape of the kernels that give every atom 16 lanes (pc_guidance, mesh_classify, mesh_pull); a cloud staged in LDS
dim3 guide_grid(int64_t N) { return dim3((unsigned)((N * 16 + 255) / 256)); }
size_t cloud_lds_bytes(int64_t n_points) { return (size_t)n_points * 24; }
// chain parameters of a stand-alone application: one step, always guided (callers pass t_first = grad_step + 1, no step counter)
ChainParams guide_alone_params(uint64_t seed, const double *d_draws) {
    ChainParams cp{};
    cp.seed = seed; cp.guide_draws = d_draws; cp.step_base = 0;
    return cp;
}

// ---- guidance per group of molecules (point clouds, meshes): host side
// workgroups of the kernels that run per group: the sum over the groups of ceil(n_g / 16) is at most floor(N / 16) + G
unsigned groups_grid(int64_t N, int n_groups) { return (unsigned)(N / 16 + n_groups); }

PcGroupsArgs groups_args(const shapemol_ctx *c, float *d_pos, int64_t N, const int *step_cur, int t_first) {
    const int G1 = c->gg_groups + 1;
    PcGroupsArgs a{};
    a.pred_pos = d_pos; a.clouds = c->gg_clouds; a.cloud_off = c->gg_ints + G1; a.radius = c->gg_radius; a.atom_off = c->gg_ints + 2 * G1;
    a.wg_table = c->gg_table; a.cp = c->chain_params; a.step_cur = step_cur;
    a.n_atoms = (int)N; a.t_first = t_first; a.grad_step = c->gg_grad_step; a.ratio = 0.2;
    return a;
}

// the per-workgroup table of this chain (atom ranges come from the batch vector on the device); ints = the installed set's
// [mol_off | cloud_off | atom_off | wg_off], G + 1 each (cloud groups or mesh groups: one table serves whichever guides)
int groups_table(shapemol_ctx *c, hipStream_t s, const int64_t *d_batch, int64_t N, int *ints, int n_groups) {
    const int64_t n_wg = groups_grid(N, n_groups);
    if (n_wg > c->gg_table_cap) {
        c->drop_graphs();                        // a captured step holds the table's address
        if (c->gg_table) { hipFree(c->gg_table); c->gg_table = nullptr; }
        c->gg_table_cap = 0;
        HIPCHK(hipMalloc((void **)&c->gg_table, (size_t)n_wg * sizeof(int2)));
        c->gg_table_cap = n_wg;
    }
    const int G1 = n_groups + 1;
    LAUNCH("prep", SMK(pc_groups_table_kernel, dim3(1), dim3(256), 0, s, d_batch, (int)N, ints, ints + G1, n_groups,
                       ints + 2 * G1, ints + 3 * G1, c->gg_table, (int)n_wg));
    return 0;
}

MeshGroupsArgs mesh_groups_args(const shapemol_ctx *c, float *d_pos, int64_t N, const int *step_cur, int t_first) {
    const int G1 = c->mg_groups + 1;
    MeshGroupsArgs a{};
    a.pred_pos = d_pos; a.clouds = c->mg_clouds; a.faces = c->mg_faces; a.fbox = c->mg_fbox; a.bounds = c->mg_bounds;
    a.cloud_off = c->mg_ints + G1; a.atom_off = c->mg_ints + 2 * G1; a.face_off = c->mg_ints + 4 * G1; a.wg_table = c->gg_table;
    a.within = c->m_within; a.out_list = c->m_out; a.cnt = c->m_cnt; a.group_flags = c->m_cnt + 4 * c->m_cnt_cap;
    a.status = c->status; a.cp = c->chain_params;
    a.step_cur = step_cur; a.n_atoms = (int)N; a.t_first = t_first; a.grad_step = c->mg_grad_step;
    return a;
}

// ---- mesh shape guidance: host side
// Validates the mesh and the cloud and builds the device image [faces F | face boxes F | cloud P] (vertices projected once,
// in the same operations as the device's mesh_project); bounds = (umin, umax, vmin, vmax, wmax) of the projected mesh.
int mesh_image(const double *h_verts, int64_t n_verts, const int32_t *h_faces, int64_t n_faces, const double *h_cloud,
                      int64_t n_cloud, const char *who, std::vector<unsigned char> &img, double (&bounds)[5]) {
    if (!h_verts || !h_faces || !h_cloud) return fail(std::string(who) + ": vertices, faces and cloud are required");
    if (n_verts < 3 || n_verts > (1 << 26)) return fail(std::string(who) + ": the mesh needs 3 .. 2^26 vertices");
    if (n_faces < 1 || n_faces > (1 << 24)) return fail(std::string(who) + ": the mesh needs 1 .. 2^24 faces");
    if (n_cloud < 3 || n_cloud > 2048) return fail(std::string(who) + ": the cloud needs 3 .. 2048 points (it is staged in LDS)");
    std::vector<double> pu(n_verts), pv(n_verts), pw(n_verts);
    for (int64_t i = 0; i < n_verts; ++i) {
        const double x = h_verts[i * 3], y = h_verts[i * 3 + 1], z = h_verts[i * 3 + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) return fail(std::string(who) + ": a vertex is not finite");
        mesh_project(x, y, z, pu[i], pv[i], pw[i]);
    }
    for (int64_t i = 0; i < n_cloud * 3; ++i)
        if (!std::isfinite(h_cloud[i])) return fail(std::string(who) + ": a cloud point is not finite");
    const size_t fb = (size_t)n_faces * sizeof(MeshFace), bb = (size_t)n_faces * sizeof(double4), cb = (size_t)n_cloud * 24;
    img.assign(fb + bb + cb, 0);
    MeshFace *faces = reinterpret_cast<MeshFace *>(img.data());
    double4 *box = reinterpret_cast<double4 *>(img.data() + fb);
    std::memcpy(img.data() + fb + bb, h_cloud, cb);
    bounds[0] = bounds[2] = INFINITY; bounds[1] = bounds[3] = bounds[4] = -INFINITY;
    for (int64_t f = 0; f < n_faces; ++f) {
        const int32_t *ix = h_faces + f * 3;
        for (int k = 0; k < 3; ++k)
            if (ix[k] < 0 || ix[k] >= n_verts) return fail(std::string(who) + ": face " + std::to_string(f) + " names a vertex outside [0, n_verts)");
        if (ix[0] == ix[1] || ix[1] == ix[2] || ix[2] == ix[0]) return fail(std::string(who) + ": face " + std::to_string(f) + " repeats a vertex");
        MeshFace &m = faces[f];
        double4 &b = box[f];
        b = make_double4(INFINITY, -INFINITY, INFINITY, -INFINITY);
        m.canon = 0;
        for (int k = 0; k < 3; ++k) {
            m.u[k] = pu[ix[k]]; m.v[k] = pv[ix[k]]; m.w[k] = pw[ix[k]];
            if (ix[k] < ix[k == 2 ? 0 : k + 1]) m.canon |= 1 << k;
            b.x = std::min(b.x, m.u[k]); b.y = std::max(b.y, m.u[k]); b.z = std::min(b.z, m.v[k]); b.w = std::max(b.w, m.v[k]);
            bounds[4] = std::max(bounds[4], m.w[k]);
        }
        bounds[0] = std::min(bounds[0], b.x); bounds[1] = std::max(bounds[1], b.y);
        bounds[2] = std::min(bounds[2], b.z); bounds[3] = std::max(bounds[3], b.w);
    }
    return 0;
}

// where a mesh, its per-step lists and its flags live: in a context, or in the temporary block of shapemol_mesh_guidance
struct MeshView {
    const MeshFace *faces; const double4 *fbox; const double *cloud; int64_t n_faces, n_points;
    float4 *within; int *out, *cnt, *status; const ChainParams *cp; const double *bounds;
};
MeshView mesh_view(const shapemol_ctx *c) {
    return {c->m_faces, c->m_fbox, c->m_cloud, c->m_nfaces, c->m_points, c->m_within, c->m_out, c->m_cnt, c->status, c->chain_params, c->m_bounds};
}
MeshGuideArgs mesh_args(const MeshView &m, float *pos, int64_t N, const int *step_cur, int t_first, int grad_step) {
    MeshGuideArgs a{};
    a.pred_pos = pos; a.cloud = m.cloud; a.faces = m.faces; a.fbox = m.fbox;
    a.within = m.within; a.out_list = m.out; a.cnt = m.cnt; a.status = m.status; a.cp = m.cp;
    a.step_cur = step_cur; a.n_atoms = (int)N; a.n_points = (int)m.n_points; a.n_faces = (int)m.n_faces;
    a.t_first = t_first; a.grad_step = grad_step;
    a.umin = m.bounds[0]; a.umax = m.bounds[1]; a.vmin = m.bounds[2]; a.vmax = m.bounds[3]; a.wmax = m.bounds[4];
    return a;
}

// the per-step lists of mesh guidance for N atoms: [within N | outmesh N | counters 4 per group (one group: the single mesh) |
// unguided-step count 1 per group (mesh groups)]; mesh_counters_clear zeroes the last two for a chain of n_groups
int mesh_workspace(shapemol_ctx *c, int64_t N, int64_t n_groups) {
    if (N <= c->m_cap && n_groups <= c->m_cnt_cap) return 0;
    N = std::max(N, c->m_cap); n_groups = std::max(n_groups, c->m_cnt_cap);
    c->drop_graphs();                            // the captured steps point into the old block
    HIPCHK(hipDeviceSynchronize());
    if (c->m_within) { hipFree(c->m_within); c->m_within = nullptr; c->m_out = c->m_cnt = nullptr; c->m_cap = c->m_cnt_cap = 0; }
    unsigned char *blk = nullptr;
    HIPCHK(hipMalloc((void **)&blk, (size_t)N * 20 + (size_t)n_groups * 20));
    c->m_within = reinterpret_cast<float4 *>(blk);
    c->m_out = reinterpret_cast<int *>(blk + (size_t)N * 16);
    c->m_cnt = reinterpret_cast<int *>(blk + (size_t)N * 20);
    c->m_cap = N; c->m_cnt_cap = n_groups;
    return 0;
}
int mesh_counters_clear(shapemol_ctx *c, hipStream_t s, int64_t n_groups) {
    HIPCHK(hipMemsetAsync(c->m_cnt, 0, (size_t)n_groups * 4 * sizeof(int), s));
    HIPCHK(hipMemsetAsync(c->m_cnt + 4 * c->m_cnt_cap, 0, (size_t)n_groups * sizeof(int), s));
    c->mg_flag_groups = n_groups;
    return 0;
}

// The launches of one kind of guidance on `pos` (Cfg and None: nothing here -- classifier-free guidance is part of the score
// evaluations and the posterior step).  In a chain step_cur is the device's step counter and t_first = T - 1; a stand-alone
// application passes no counter and t_first = grad_step + 1.
int enqueue_guidance(shapemol_ctx *c, hipStream_t s, Guide kind, float *pos, int64_t N, const int *step_cur, int t_first) {
    if (kind == Guide::Mesh) {
        const MeshGuideArgs ma = mesh_args(mesh_view(c), pos, N, step_cur, t_first, c->m_grad_step);
        LAUNCH("mesh_classify", SMK(mesh_classify_kernel, guide_grid(N), dim3(256), mesh_lds_bytes((int)c->m_points), s, ma));
        LAUNCH("mesh_pull", SMK(mesh_pull_kernel, guide_grid(N), dim3(256), mesh_lds_bytes((int)c->m_points), s, ma));
    } else if (kind == Guide::MeshGroups) {  // each group of molecules against its own mesh
        const MeshGroupsArgs ma = mesh_groups_args(c, pos, N, step_cur, t_first);
        const dim3 grid(groups_grid(N, c->mg_groups));
        LAUNCH("mesh_classify_groups", SMK(mesh_classify_groups_kernel, grid, dim3(256), mesh_groups_lds_bytes(c->mg_max_points), s, ma));
        LAUNCH("mesh_pull_groups", SMK(mesh_pull_groups_kernel, grid, dim3(256), mesh_groups_lds_bytes(c->mg_max_points), s, ma));
    } else if (kind == Guide::Cloud) {
        PcGuideArgs ga{pos, c->g_cloud, c->chain_params, step_cur, (int)N, (int)c->g_points, t_first, c->g_grad_step, c->g_radius, 0.2};
        LAUNCH("pc_guidance", SMK(pc_guidance_kernel, guide_grid(N), dim3(256), cloud_lds_bytes(c->g_points), s, ga));
    } else if (kind == Guide::Groups) {     // each group of molecules towards its own cloud
        const PcGroupsArgs ga = groups_args(c, pos, N, step_cur, t_first);
        LAUNCH("pc_guidance_groups", SMK(pc_guidance_groups_kernel, dim3(groups_grid(N, c->gg_groups)), dim3(256), cloud_lds_bytes(c->gg_max_points), s, ga));
    }
    return 0;
}

// shapemol_guide_points*: one always-guided application of the context's guidance of `kind` to given positions
int guide_alone(shapemol_ctx *c, hipStream_t s, Guide kind, float *d_pos, int64_t N, const double *d_draws, uint64_t seed) {
    LAUNCH("prep", SMK(set_chain_params_kernel, dim3(1), dim3(1), 0, s, c->chain_params, guide_alone_params(seed, d_draws), c->steps));
    const int grad_step = kind == Guide::Mesh ? c->m_grad_step : (kind == Guide::MeshGroups ? c->mg_grad_step :
                          (kind == Guide::Cloud ? c->g_grad_step : c->gg_grad_step));
    return enqueue_guidance(c, s, kind, d_pos, N, nullptr, grad_step + 1);
}

void mesh_groups_clear(shapemol_ctx *c) {
    if (c->mg_faces) { hipFree(c->mg_faces); c->mg_faces = nullptr; }
    c->mg_fbox = nullptr; c->mg_clouds = c->mg_bounds = nullptr; c->mg_ints = nullptr;
    c->mg_groups = 0; c->mg_max_points = 0; c->mg_mols = 0; c->mg_nfaces = 0; c->mg_draws = nullptr;
}

void mesh_single_clear(shapemol_ctx *c) {
    if (c->m_faces) { hipFree(c->m_faces); c->m_faces = nullptr; c->m_fbox = nullptr; c->m_cloud = nullptr; }
    c->m_nfaces = 0; c->m_points = 0; c->m_draws = nullptr;
}

void groups_clear(shapemol_ctx *c) {
    if (c->gg_clouds) { hipFree(c->gg_clouds); c->gg_clouds = nullptr; }
    c->gg_radius = nullptr; c->gg_ints = nullptr;
    c->gg_groups = 0; c->gg_max_points = 0; c->gg_mols = 0; c->gg_points = 0; c->gg_draws = nullptr;
}

}  // namespace

extern "C" {

int shapemol_set_guidance(shapemol_ctx *c, const double *h_cloud, int64_t n_points, double radius, int32_t grad_step, const double *d_draws) {
    if (!c) return fail("shapemol_set_guidance: null ctx");
    if (n_points < 0 || n_points > 2048 || (n_points > 0 && n_points < 3)) return fail("shapemol_set_guidance: the cloud needs 3 .. 2048 points (it is staged in LDS)");
    if (n_points > 0 && (!h_cloud || !(radius > 0.0))) return fail("shapemol_set_guidance: cloud / radius missing");
    HIPCHK(hipSetDevice(c->device));
    c->drop_graphs();                            // also drains the device: the old cloud may still be in use
    if (c->g_cloud) { hipFree(c->g_cloud); c->g_cloud = nullptr; }
    c->g_points = 0; c->g_draws = nullptr;
    if (n_points == 0) return 0;
    groups_clear(c);                             // a single cloud replaces clouds per group
    HIPCHK(hipMalloc((void **)&c->g_cloud, (size_t)n_points * 3 * sizeof(double)));
    HIPCHK(hipMemcpy(c->g_cloud, h_cloud, (size_t)n_points * 3 * sizeof(double), hipMemcpyHostToDevice));
    c->g_points = n_points; c->g_radius = radius; c->g_grad_step = grad_step; c->g_draws = d_draws;
    return 0;
}

int shapemol_set_guidance_groups(shapemol_ctx *c, int32_t n_groups, const int64_t *h_mol_off, const double *h_clouds, const int64_t *h_cloud_off,
                                 const double *h_radius, int32_t grad_step, const double *d_draws) {
    const std::string me = "shapemol_set_guidance_groups: ";
    if (!c) return fail(me + "null ctx");
    if (n_groups < 0 || n_groups > (1 << 20)) return fail(me + "n_groups out of range");
    if (n_groups > 0) {
        if (!h_mol_off || !h_cloud_off || !h_radius) return fail(me + "offsets / radii missing");
        if (h_mol_off[0] != 0 || h_cloud_off[0] != 0) return fail(me + "group 0: the molecule and cloud offsets must start at 0");
        for (int g = 0; g < n_groups; ++g) {
            const std::string grp = me + "group " + std::to_string(g) + ": ";
            if (h_mol_off[g + 1] < h_mol_off[g]) return fail(grp + "the molecule offsets decrease");
            if (h_cloud_off[g + 1] < h_cloud_off[g]) return fail(grp + "the cloud offsets decrease");
            const int64_t p = h_cloud_off[g + 1] - h_cloud_off[g];
            if (p > 0 && (p < 3 || p > 2048)) return fail(grp + "the cloud needs 3 .. 2048 points (it is staged in LDS), or none");
            if (p > 0 && !(h_radius[g] > 0.0)) return fail(grp + "the radius must be > 0");
        }
        if (h_mol_off[n_groups] > (1 << 27)) return fail(me + "too many molecules");
        if (h_cloud_off[n_groups] > 0 && !h_clouds) return fail(me + "clouds missing");
    }
    HIPCHK(hipSetDevice(c->device));
    c->drop_graphs();                            // also drains the device: the old clouds may still be in use
    groups_clear(c);
    if (n_groups == 0) return 0;
    if (c->g_cloud) { hipFree(c->g_cloud); c->g_cloud = nullptr; }      // clouds per group replace a single cloud
    c->g_points = 0; c->g_draws = nullptr;
    const int G1 = n_groups + 1;
    const int64_t P = h_cloud_off[n_groups];
    std::vector<double> hd((size_t)P * 3 + n_groups);
    if (P) std::copy(h_clouds, h_clouds + P * 3, hd.begin());
    std::copy(h_radius, h_radius + n_groups, hd.begin() + P * 3);
    std::vector<int> hi((size_t)4 * G1, 0);       // mol_off | cloud_off | atom_off | wg_off (the last two are written on the device)
    int max_points = 0;
    for (int g = 0; g < G1; ++g) { hi[g] = (int)h_mol_off[g]; hi[G1 + g] = (int)h_cloud_off[g]; }
    for (int g = 0; g < n_groups; ++g) max_points = std::max(max_points, hi[G1 + g + 1] - hi[G1 + g]);
    const size_t bytes_d = hd.size() * sizeof(double), bytes_i = hi.size() * sizeof(int);
    HIPCHK(hipMalloc((void **)&c->gg_clouds, bytes_d + bytes_i));
    HIPCHK(hipMemcpy(c->gg_clouds, hd.data(), bytes_d, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((char *)c->gg_clouds + bytes_d, hi.data(), bytes_i, hipMemcpyHostToDevice));
    c->gg_radius = c->gg_clouds + P * 3; c->gg_ints = (int *)((char *)c->gg_clouds + bytes_d);
    c->gg_groups = n_groups; c->gg_max_points = max_points; c->gg_mols = h_mol_off[n_groups]; c->gg_points = P;
    c->gg_grad_step = grad_step; c->gg_draws = d_draws;
    return 0;
}

int shapemol_guide_points_groups(shapemol_ctx *c, float *d_pos, const int64_t *d_batch, int64_t N, const double *d_draws, uint64_t seed,
                                 void *stream) {
    if (!c || !d_pos || !d_batch || N < 1 || N > (1 << 27)) return fail("shapemol_guide_points_groups: bad argument");
    if (c->gg_groups <= 0) return fail("shapemol_guide_points_groups: no groups set (shapemol_set_guidance_groups)");
    HIPCHK(hipSetDevice(c->device));
    if (ensure_workspace(c, N, 1)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (c->gg_points == 0) return 0;             // no group has a cloud: nothing moves
    if (groups_table(c, s, d_batch, N, c->gg_ints, c->gg_groups)) return 1;
    return guide_alone(c, s, Guide::Groups, d_pos, N, d_draws, seed);
}

int shapemol_guide_points(shapemol_ctx *c, float *d_pos, int64_t N, const double *d_draws, uint64_t seed, void *stream) {
    if (!c || !d_pos || N < 1) return fail("shapemol_guide_points: bad argument");
    if (c->g_points <= 0) return fail("shapemol_guide_points: no cloud set (shapemol_set_guidance)");
    HIPCHK(hipSetDevice(c->device));
    if (ensure_workspace(c, std::max<int64_t>(N, 1), 1)) return 1;
    return guide_alone(c, (hipStream_t)stream, Guide::Cloud, d_pos, N, d_draws, seed);
}

int shapemol_pointcloud_guidance(const double *h_cloud, int64_t n_points, double radius, double ratio, float *d_pos, int64_t N,
                                 const double *d_draws, uint64_t seed, void *stream) {
    if (!h_cloud || !d_pos || N < 1) return fail("shapemol_pointcloud_guidance: bad argument");
    if (n_points < 3 || n_points > 2048) return fail("shapemol_pointcloud_guidance: the cloud needs 3 .. 2048 points (it is staged in LDS)");
    if (!(radius > 0.0) || !(ratio >= 0.0 && ratio < 0.8)) return fail("shapemol_pointcloud_guidance: radius must be > 0, ratio in [0, 0.8)");
    hipStream_t s = (hipStream_t)stream;
    const size_t cloud_bytes = (size_t)n_points * 3 * sizeof(double);
    unsigned char *blk = nullptr;                       // [cloud | ChainParams | step counter]
    HIPCHK(hipMalloc((void **)&blk, cloud_bytes + sizeof(ChainParams) + 16));
    double *d_cloud = reinterpret_cast<double *>(blk);
    ChainParams *d_cp = reinterpret_cast<ChainParams *>(blk + cloud_bytes);
    int *d_step = reinterpret_cast<int *>(blk + cloud_bytes + sizeof(ChainParams));
    hipError_t e = hipMemcpyAsync(d_cloud, h_cloud, cloud_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(set_chain_params_kernel, dim3(1), dim3(1), 0, s, d_cp, guide_alone_params(seed, d_draws), d_step);
        PcGuideArgs ga{d_pos, d_cloud, d_cp, nullptr, (int)N, (int)n_points, 1, 0, radius, ratio};      // t_first - 0 > grad_step: always guided
        hipLaunchKernelGGL(pc_guidance_kernel, guide_grid(N), dim3(256), cloud_lds_bytes(n_points), s, ga);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(s);       // the block is freed below; the reference's function is synchronous too
    hipFree(blk);
    if (e != hipSuccess) return fail(std::string("shapemol_pointcloud_guidance: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(std::string("shapemol_pointcloud_guidance: ") + hipGetErrorString(e2));
    return 0;
}

int shapemol_set_mesh_guidance(shapemol_ctx *c, const double *h_verts, int64_t n_verts, const int32_t *h_faces, int64_t n_faces,
                               const double *h_cloud, int64_t n_cloud, int32_t grad_step, const double *d_draws) {
    if (!c) return fail("shapemol_set_mesh_guidance: null ctx");
    if (n_faces < 0) return fail("shapemol_set_mesh_guidance: n_faces < 0");
    std::vector<unsigned char> img;
    double bounds[5];
    if (n_faces > 0 && mesh_image(h_verts, n_verts, h_faces, n_faces, h_cloud, n_cloud, "shapemol_set_mesh_guidance", img, bounds)) return 1;
    HIPCHK(hipSetDevice(c->device));
    c->drop_graphs();                            // also drains the device: the old mesh may still be in use
    mesh_single_clear(c);
    if (n_faces == 0) return 0;
    mesh_groups_clear(c);                        // a single mesh replaces meshes per group
    unsigned char *blk = nullptr;
    HIPCHK(hipMalloc((void **)&blk, img.size()));
    HIPCHK(hipMemcpy(blk, img.data(), img.size(), hipMemcpyHostToDevice));
    c->m_faces = reinterpret_cast<MeshFace *>(blk);
    c->m_fbox = reinterpret_cast<double4 *>(blk + (size_t)n_faces * sizeof(MeshFace));
    c->m_cloud = reinterpret_cast<double *>(blk + (size_t)n_faces * (sizeof(MeshFace) + sizeof(double4)));
    std::memcpy(c->m_bounds, bounds, sizeof(bounds));
    c->m_nfaces = n_faces; c->m_points = n_cloud; c->m_grad_step = grad_step; c->m_draws = d_draws;
    return 0;
}

int shapemol_guide_points_mesh(shapemol_ctx *c, float *d_pos, int64_t N, const double *d_draws, uint64_t seed, void *stream) {
    if (!c || !d_pos || N < 1 || N > (1 << 27)) return fail("shapemol_guide_points_mesh: bad argument");
    if (c->m_nfaces <= 0) return fail("shapemol_guide_points_mesh: no mesh set (shapemol_set_mesh_guidance)");
    HIPCHK(hipSetDevice(c->device));
    if (ensure_workspace(c, std::max<int64_t>(N, 1), 1) || mesh_workspace(c, N, 1)) return 1;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(c->m_cnt, 0, 4 * sizeof(int), s));
    HIPCHK(hipMemsetAsync(c->status + ST_MESH, 0, sizeof(int), s));
    return guide_alone(c, s, Guide::Mesh, d_pos, N, d_draws, seed);
}

int shapemol_set_mesh_guidance_groups(shapemol_ctx *c, int32_t n_groups, const int64_t *h_mol_off, const double *h_verts, const int64_t *h_vert_off,
                                      const int32_t *h_faces, const int64_t *h_face_off, const double *h_clouds, const int64_t *h_cloud_off,
                                      int32_t grad_step, const double *d_draws) {
    const std::string me = "shapemol_set_mesh_guidance_groups: ";
    if (!c) return fail(me + "null ctx");
    if (n_groups < 0 || n_groups > (1 << 20)) return fail(me + "n_groups out of range");
    // host image [faces | face boxes | clouds | bounds G x 5 | ints 5 (G + 1)]; every group's mesh goes through mesh_image, the
    // single mesh's validation and projection, with its face indices relative to the group's own vertices
    const int G1 = n_groups + 1;
    std::vector<std::vector<unsigned char>> imgs(n_groups);
    std::vector<double> hb((size_t)n_groups * 5, 0.0);
    int64_t F = 0, P = 0;
    int max_points = 0;
    if (n_groups > 0) {
        if (!h_mol_off || !h_vert_off || !h_face_off || !h_cloud_off) return fail(me + "offsets missing");
        if (h_mol_off[0] != 0 || h_vert_off[0] != 0 || h_face_off[0] != 0 || h_cloud_off[0] != 0)
            return fail(me + "group 0: the molecule, vertex, face and cloud offsets must start at 0");
        for (int g = 0; g < n_groups; ++g) {
            const std::string grp = me + "group " + std::to_string(g);
            if (h_mol_off[g + 1] < h_mol_off[g]) return fail(grp + ": the molecule offsets decrease");
            if (h_vert_off[g + 1] < h_vert_off[g]) return fail(grp + ": the vertex offsets decrease");
            if (h_face_off[g + 1] < h_face_off[g]) return fail(grp + ": the face offsets decrease");
            if (h_cloud_off[g + 1] < h_cloud_off[g]) return fail(grp + ": the cloud offsets decrease");
            const int64_t nv = h_vert_off[g + 1] - h_vert_off[g], nf = h_face_off[g + 1] - h_face_off[g], np = h_cloud_off[g + 1] - h_cloud_off[g];
            if (nv == 0 && nf == 0 && np == 0) continue;       // a group without a mesh
            if (!h_verts || !h_faces || !h_clouds) return fail(grp + ": vertices, faces and cloud are required");
            double bounds[5];
            if (mesh_image(h_verts + h_vert_off[g] * 3, nv, h_faces + h_face_off[g] * 3, nf, h_clouds + h_cloud_off[g] * 3, np, grp.c_str(), imgs[g], bounds)) return 1;
            std::copy(bounds, bounds + 5, hb.begin() + (size_t)g * 5);
            max_points = std::max(max_points, (int)np);
        }
        F = h_face_off[n_groups]; P = h_cloud_off[n_groups];
        if (h_mol_off[n_groups] > (1 << 27)) return fail(me + "too many molecules");
        if (F > (1 << 27)) return fail(me + "too many faces");
        if (P > (1 << 27) || h_vert_off[n_groups] > (1 << 27)) return fail(me + "too many cloud points / vertices");
    }
    HIPCHK(hipSetDevice(c->device));
    c->drop_graphs();                            // also drains the device: the old meshes may still be in use
    mesh_groups_clear(c);
    if (n_groups == 0) return 0;
    mesh_single_clear(c);                        // meshes per group replace a single mesh
    const size_t fb = (size_t)F * sizeof(MeshFace), bb = (size_t)F * sizeof(double4), cb = (size_t)P * 24, nb = hb.size() * sizeof(double);
    std::vector<unsigned char> img(fb + bb + cb + nb + (size_t)5 * G1 * sizeof(int), 0);
    int *hi = reinterpret_cast<int *>(img.data() + fb + bb + cb + nb);       // mol_off | cloud_off | atom_off | wg_off | face_off
    for (int g = 0; g < G1; ++g) { hi[g] = (int)h_mol_off[g]; hi[G1 + g] = (int)h_cloud_off[g]; hi[4 * G1 + g] = (int)h_face_off[g]; }
    for (int g = 0; g < n_groups; ++g) {
        if (imgs[g].empty()) continue;
        const size_t nf = (size_t)(h_face_off[g + 1] - h_face_off[g]), np = (size_t)(h_cloud_off[g + 1] - h_cloud_off[g]);
        const unsigned char *src = imgs[g].data();
        std::memcpy(img.data() + (size_t)h_face_off[g] * sizeof(MeshFace), src, nf * sizeof(MeshFace));
        std::memcpy(img.data() + fb + (size_t)h_face_off[g] * sizeof(double4), src + nf * sizeof(MeshFace), nf * sizeof(double4));
        std::memcpy(img.data() + fb + bb + (size_t)h_cloud_off[g] * 24, src + nf * (sizeof(MeshFace) + sizeof(double4)), np * 24);
    }
    std::memcpy(img.data() + fb + bb + cb, hb.data(), nb);
    unsigned char *blk = nullptr;
    HIPCHK(hipMalloc((void **)&blk, img.size()));
    HIPCHK(hipMemcpy(blk, img.data(), img.size(), hipMemcpyHostToDevice));
    c->mg_faces = reinterpret_cast<MeshFace *>(blk);
    c->mg_fbox = reinterpret_cast<double4 *>(blk + fb);
    c->mg_clouds = reinterpret_cast<double *>(blk + fb + bb);
    c->mg_bounds = reinterpret_cast<double *>(blk + fb + bb + cb);
    c->mg_ints = reinterpret_cast<int *>(blk + fb + bb + cb + nb);
    c->mg_groups = n_groups; c->mg_max_points = max_points; c->mg_mols = h_mol_off[n_groups]; c->mg_nfaces = F;
    c->mg_grad_step = grad_step; c->mg_draws = d_draws;
    return 0;
}

int shapemol_guide_points_mesh_groups(shapemol_ctx *c, float *d_pos, const int64_t *d_batch, int64_t N, const double *d_draws, uint64_t seed,
                                      void *stream) {
    if (!c || !d_pos || !d_batch || N < 1 || N > (1 << 27)) return fail("shapemol_guide_points_mesh_groups: bad argument");
    if (c->mg_groups <= 0) return fail("shapemol_guide_points_mesh_groups: no groups set (shapemol_set_mesh_guidance_groups)");
    HIPCHK(hipSetDevice(c->device));
    if (ensure_workspace(c, N, 1) || mesh_workspace(c, N, c->mg_groups)) return 1;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(c->status + ST_MESH, 0, sizeof(int), s));
    if (c->mg_nfaces == 0) return 0;             // no group has a mesh: nothing moves
    if (mesh_counters_clear(c, s, c->mg_groups)) return 1;
    if (groups_table(c, s, d_batch, N, c->mg_ints, c->mg_groups)) return 1;
    return guide_alone(c, s, Guide::MeshGroups, d_pos, N, d_draws, seed);
}

int shapemol_mesh_guidance(const double *h_verts, int64_t n_verts, const int32_t *h_faces, int64_t n_faces, const double *h_cloud,
                           int64_t n_cloud, float *d_pos, int64_t N, const double *d_draws, uint64_t seed, int32_t *flag_out,
                           void *stream) {
    if (flag_out) *flag_out = 0;
    if (!d_pos || N < 1 || N > (1 << 27)) return fail("shapemol_mesh_guidance: bad argument");
    std::vector<unsigned char> img;
    double bounds[5];
    if (mesh_image(h_verts, n_verts, h_faces, n_faces, h_cloud, n_cloud, "shapemol_mesh_guidance", img, bounds)) return 1;
    hipStream_t s = (hipStream_t)stream;
    // [mesh image | ChainParams | step counter, status [8], counters [4] | within N | outmesh N]
    const size_t o_cp = (img.size() + 255) / 256 * 256, o_st = o_cp + (sizeof(ChainParams) + 255) / 256 * 256;
    const size_t o_in = o_st + 256, o_out = o_in + (size_t)N * 16, total = o_out + (size_t)N * 4;
    unsigned char *blk = nullptr;
    HIPCHK(hipMalloc((void **)&blk, total));
    int *d_misc = reinterpret_cast<int *>(blk + o_st);        // [0] step counter, [4 .. 11] status, [16 .. 19] counters
    hipError_t e = hipMemcpyAsync(blk, img.data(), img.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_misc, 0, 256, s);
    int32_t flag = 0;
    if (e == hipSuccess) {
        ChainParams *d_cp = reinterpret_cast<ChainParams *>(blk + o_cp);
        hipLaunchKernelGGL(set_chain_params_kernel, dim3(1), dim3(1), 0, s, d_cp, guide_alone_params(seed, d_draws), d_misc);
        const MeshView mv{reinterpret_cast<const MeshFace *>(blk), reinterpret_cast<const double4 *>(blk + (size_t)n_faces * sizeof(MeshFace)),
                          reinterpret_cast<const double *>(blk + (size_t)n_faces * (sizeof(MeshFace) + sizeof(double4))), n_faces, n_cloud,
                          reinterpret_cast<float4 *>(blk + o_in), reinterpret_cast<int *>(blk + o_out), d_misc + 16, d_misc + 4, d_cp, bounds};
        const MeshGuideArgs a = mesh_args(mv, d_pos, N, nullptr, 1, 0);      // t_first - 0 > grad_step: always guided
        hipLaunchKernelGGL(mesh_classify_kernel, guide_grid(N), dim3(256), mesh_lds_bytes((int)n_cloud), s, a);
        hipLaunchKernelGGL(mesh_pull_kernel, guide_grid(N), dim3(256), mesh_lds_bytes((int)n_cloud), s, a);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_misc + 4 + ST_MESH, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    }
    const hipError_t e2 = hipStreamSynchronize(s);       // the block is freed below; the reference's function is synchronous too
    hipFree(blk);
    if (e != hipSuccess) return fail(std::string("shapemol_mesh_guidance: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(std::string("shapemol_mesh_guidance: ") + hipGetErrorString(e2));
    if (flag) {
        if (flag_out) *flag_out = 1;
        return fail("mesh shape guidance: fewer than 3 atoms lie inside the mesh and > 0.4 from the cloud (none at all, or fewer "
                    "than 3 while atoms are to be pulled); the reference raises ValueError from its KD-tree here");
    }
    return 0;
}

}  // extern "C"
