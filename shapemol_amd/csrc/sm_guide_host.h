// Host side of the guidance of a chain's predicted x0: which kind a chain uses (chain_guide), the launches of every kind
// (enqueue_guidance), their device data (setters) and the stand-alone entry points of the C ABI.  Included by
// shapemol_hip.hip behind shapemol_ctx and the LAUNCH / SMK macros.
//
// Shape guidance has one form per kind: a SET of groups of molecules, each group with its own cloud (CloudSet) or mesh
// (MeshSet).  The single-cloud / single-mesh entry points use a set of one group marked `whole`: it spans whatever batch comes,
// so it needs no batch vector (its atoms are [0, N)) and carries no molecule count to check.
#pragma once

// shape_decoder.hip: the decoder context's side of field guidance
extern "C" {
void shapemol_sd_describe_(const shapemol_sd_ctx *c, int *device, int *latent);
int shapemol_sd_chain_prepare_(shapemol_sd_ctx *c, const float *d_z, int64_t n_shapes, hipStream_t s, uint64_t *gen);
int shapemol_sd_chain_guide_(shapemol_sd_ctx *c, float *pos, const int *mol_of, const int *mol_off, int64_t n_atoms, int64_t n_shapes, double grad_lr,
                             const int *step_cur, int t_first, int grad_step, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
}

namespace {

// The guidance of the chains to come: the reference's if / elif in sample_diffusion -- mesh, else the point cloud, else the
// decoder's field (`use_grad`), else classifier-free guidance.  Groups without any mesh / cloud guide nothing (and leave the next kind its turn).  The only place
// that spells this out.
Guide chain_guide(const shapemol_ctx *c) {
    if (c->ms.nfaces > 0) return Guide::Mesh;
    if (c->cs.points > 0) return Guide::Cloud;
    // (a field whose gate `t > grad_step` no step of the chain passes launches nothing: the chain is the unguided one, bit for bit.
    // It still takes the branch, as the reference's `elif use_grad:` does: classifier-free guidance does not get its turn)
    if (c->field_sd) return c->cfg.num_timesteps - 1 - c->first_step > c->field_step ? Guide::Field : Guide::None;
    return c->cfg_w != 0.0 || c->cgs.groups > 0 ? Guide::Cfg : Guide::None;
}

// workgroups of the guidance kernels (16 atoms x 16 lanes each, every workgroup within one group): the sum over the groups of
// ceil(n_g / 16) is at most floor(N / 16) + G
unsigned groups_grid(int64_t N, int n_groups) { return (unsigned)(N / 16 + n_groups); }
size_t cloud_lds_bytes(int64_t n_points) { return (size_t)n_points * 24; }
// chain parameters of a stand-alone application: one step, always guided (callers pass t_first = grad_step + 1, no step counter)
ChainParams guide_alone_params(uint64_t seed, const double *d_draws) {
    ChainParams cp{};
    cp.seed = seed; cp.guide_draws = d_draws; cp.step_base = 0;
    return cp;
}

PcGroupsArgs cloud_args(const CloudSet &cs, const int2 *table, const ChainParams *cp, float *d_pos, int64_t N, const int *step_cur, int t_first) {
    const int G1 = cs.groups + 1;
    PcGroupsArgs a{};
    a.pred_pos = d_pos; a.clouds = cs.clouds; a.cloud_off = cs.ints + G1; a.radius = cs.radius; a.atom_off = cs.ints + 2 * G1;
    a.wg_table = table; a.cp = cp; a.step_cur = step_cur;
    a.n_atoms = (int)N; a.t_first = t_first; a.grad_step = cs.grad_step; a.ratio = 0.2;
    return a;
}

// within / out_list [N], cnt [G][2][2], flags [G]: the per-step lists (mesh_workspace, or the block of shapemol_mesh_guidance)
MeshGroupsArgs mesh_args(const MeshSet &ms, const int2 *table, float4 *within, int *out_list, int *cnt, int *flags, int *status,
                         const ChainParams *cp, float *d_pos, int64_t N, const int *step_cur, int t_first) {
    const int G1 = ms.groups + 1;
    MeshGroupsArgs a{};
    a.pred_pos = d_pos; a.clouds = ms.clouds; a.faces = ms.faces; a.fbox = ms.fbox; a.bounds = ms.bounds;
    a.cloud_off = ms.ints + G1; a.atom_off = ms.ints + 2 * G1; a.face_off = ms.ints + 4 * G1; a.wg_table = table;
    a.within = within; a.out_list = out_list; a.cnt = cnt; a.group_flags = flags; a.status = status; a.cp = cp;
    a.step_cur = step_cur; a.n_atoms = (int)N; a.t_first = t_first; a.grad_step = ms.grad_step;
    return a;
}

// the per-workgroup table of this chain (atom ranges come from the batch vector on the device; d_batch = nullptr for a `whole`
// set: one group, atoms [0, N)); ints = the installed set's [mol_off | cloud_off | atom_off | wg_off], G + 1 each (cloud groups
// or mesh groups: one table serves whichever guides)
int groups_table(shapemol_ctx *c, hipStream_t s, const int64_t *d_batch, int64_t N, int *ints, int n_groups) {
    const int64_t n_wg = groups_grid(N, n_groups);
    if (n_wg > c->wg_table_cap) c->drop_graphs();      // a captured step holds the table's address
    HIPCHK(grow(c->mem_wg, {dev_buf(&c->wg_table, (size_t)n_wg * sizeof(int2))}, c->wg_table_cap, n_wg));
    const int G1 = n_groups + 1;
    LAUNCH("prep", SMK(pc_groups_table_kernel, dim3(1), dim3(256), 0, s, d_batch, (int)N, ints, ints + G1, n_groups,
                       ints + 2 * G1, ints + 3 * G1, c->wg_table, (int)n_wg));
    return 0;
}

// ---- point-cloud guidance: host side
template <typename Set>          // CloudSet or MeshSet with the list that owns its block: nothing installed
void set_clear(DevList &mem, Set &set) { mem.release(); set = Set{}; }

// Installs groups that the caller has validated into a cleared set: one device block of `mem` [clouds | radii | mol_off,
// cloud_off, atom_off, wg_off (G + 1 ints each)], rounded up to 256 bytes, and `tail_bytes` more behind it for the caller (*tail).
int cloud_set_install(DevList &mem, CloudSet &cs, int n_groups, const int64_t *h_mol_off, const double *h_clouds, const int64_t *h_cloud_off,
                      const double *h_radius, bool whole, int grad_step, const double *d_draws, size_t tail_bytes = 0,
                      unsigned char **tail = nullptr) {
    const int G1 = n_groups + 1;
    const int64_t P = h_cloud_off[n_groups];
    std::vector<double> hd((size_t)P * 3 + n_groups);
    if (P) std::copy(h_clouds, h_clouds + P * 3, hd.begin());
    std::copy(h_radius, h_radius + n_groups, hd.begin() + P * 3);
    std::vector<int> hi((size_t)4 * G1, 0);       // mol_off | cloud_off | atom_off | wg_off (the last two are written on the device)
    int max_points = 0;
    for (int g = 0; g < G1; ++g) { hi[g] = (int)h_mol_off[g]; hi[G1 + g] = (int)h_cloud_off[g]; }
    for (int g = 0; g < n_groups; ++g) max_points = std::max(max_points, hi[G1 + g + 1] - hi[G1 + g]);
    const size_t bytes_d = hd.size() * sizeof(double), bytes_i = hi.size() * sizeof(int), bytes = (bytes_d + bytes_i + 255) / 256 * 256;
    HIPCHK(mem.alloc(&cs.clouds, bytes + tail_bytes));
    hipError_t e = hipMemcpy(cs.clouds, hd.data(), bytes_d, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char *)cs.clouds + bytes_d, hi.data(), bytes_i, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_clear(mem, cs); return hip_fail("guidance clouds: hipMemcpy", e); }
    cs.radius = cs.clouds + P * 3; cs.ints = (int *)((char *)cs.clouds + bytes_d);
    cs.groups = n_groups; cs.max_points = max_points; cs.mols = h_mol_off[n_groups]; cs.points = P; cs.whole = whole;
    cs.grad_step = grad_step; cs.draws = d_draws;
    if (tail) *tail = (unsigned char *)cs.clouds + bytes;
    return 0;
}

// the single-cloud entry points: ONE group of n_points that spans whatever batch comes (`whole`: no molecule count)
int cloud_set_install_whole(DevList &mem, CloudSet &cs, const double *h_cloud, int64_t n_points, double radius, int grad_step, const double *d_draws,
                            size_t tail_bytes = 0, unsigned char **tail = nullptr) {
    const int64_t mol_off[2] = {0, 0}, cloud_off[2] = {0, n_points};
    return cloud_set_install(mem, cs, 1, mol_off, h_cloud, cloud_off, &radius, true, grad_step, d_draws, tail_bytes, tail);
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

// host image of a set of mesh groups: [faces | face boxes | clouds | bounds G x 5 | mol_off, cloud_off, atom_off, wg_off,
// face_off (G + 1 ints each)]
struct MeshSetImage { std::vector<unsigned char> bytes; int64_t F = 0, P = 0, mols = 0; int groups = 0, max_points = 0; bool whole = false; };

// Validates the groups and builds their image; every group's mesh goes through mesh_image, with its face indices relative to
// the group's own vertices.  `whole`: the one group of the single-mesh entry point `me`, whose errors name no group.
int mesh_set_image(const std::string &me, bool whole, int n_groups, const int64_t *h_mol_off, const double *h_verts, const int64_t *h_vert_off,
                   const int32_t *h_faces, const int64_t *h_face_off, const double *h_clouds, const int64_t *h_cloud_off, MeshSetImage &out) {
    const int G1 = n_groups + 1;
    std::vector<std::vector<unsigned char>> imgs(n_groups);
    std::vector<double> hb((size_t)n_groups * 5, 0.0);
    int max_points = 0;
    if (!whole) {
        if (!h_mol_off || !h_vert_off || !h_face_off || !h_cloud_off) return fail(me + ": offsets missing");
        if (h_mol_off[0] != 0 || h_vert_off[0] != 0 || h_face_off[0] != 0 || h_cloud_off[0] != 0)
            return fail(me + ": group 0: the molecule, vertex, face and cloud offsets must start at 0");
    }
    for (int g = 0; g < n_groups; ++g) {
        const std::string grp = whole ? me : me + ": group " + std::to_string(g);
        const int64_t nv = h_vert_off[g + 1] - h_vert_off[g], nf = h_face_off[g + 1] - h_face_off[g], np = h_cloud_off[g + 1] - h_cloud_off[g];
        if (!whole) {
            if (h_mol_off[g + 1] < h_mol_off[g]) return fail(grp + ": the molecule offsets decrease");
            if (nv < 0) return fail(grp + ": the vertex offsets decrease");
            if (nf < 0) return fail(grp + ": the face offsets decrease");
            if (np < 0) return fail(grp + ": the cloud offsets decrease");
            if (nv == 0 && nf == 0 && np == 0) continue;       // a group without a mesh
        }
        double bounds[5];
        if (mesh_image(h_verts ? h_verts + h_vert_off[g] * 3 : nullptr, nv, h_faces ? h_faces + h_face_off[g] * 3 : nullptr, nf,
                       h_clouds ? h_clouds + h_cloud_off[g] * 3 : nullptr, np, grp.c_str(), imgs[g], bounds)) return 1;
        std::copy(bounds, bounds + 5, hb.begin() + (size_t)g * 5);
        max_points = std::max(max_points, (int)np);
    }
    const int64_t F = h_face_off[n_groups], P = h_cloud_off[n_groups];
    if (h_mol_off[n_groups] > (1 << 27)) return fail(me + ": too many molecules");
    if (F > (1 << 27)) return fail(me + ": too many faces");
    if (P > (1 << 27) || h_vert_off[n_groups] > (1 << 27)) return fail(me + ": too many cloud points / vertices");
    const size_t fb = (size_t)F * sizeof(MeshFace), bb = (size_t)F * sizeof(double4), cb = (size_t)P * 24, nb = hb.size() * sizeof(double);
    std::vector<unsigned char> &img = out.bytes;
    img.assign(fb + bb + cb + nb + (size_t)5 * G1 * sizeof(int), 0);
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
    out.F = F; out.P = P; out.mols = h_mol_off[n_groups]; out.groups = n_groups; out.max_points = max_points; out.whole = whole;
    return 0;
}

// the single-mesh entry point `me`: ONE group that spans whatever batch comes (`whole`: no molecule count, errors name no group)
int mesh_set_image_whole(const std::string &me, const double *h_verts, int64_t n_verts, const int32_t *h_faces, int64_t n_faces,
                         const double *h_cloud, int64_t n_cloud, MeshSetImage &out) {
    const int64_t mol_off[2] = {0, 0}, vert_off[2] = {0, n_verts}, face_off[2] = {0, n_faces}, cloud_off[2] = {0, n_cloud};
    return mesh_set_image(me, true, 1, mol_off, h_verts, vert_off, h_faces, face_off, h_cloud, cloud_off, out);
}

// into a cleared set: one device block of `mem`, the image, rounded up to 256 bytes, and `tail_bytes` more behind it for the caller (*tail)
int mesh_set_install(DevList &mem, MeshSet &ms, const MeshSetImage &im, int grad_step, const double *d_draws, size_t tail_bytes = 0, unsigned char **tail = nullptr) {
    const size_t fb = (size_t)im.F * sizeof(MeshFace), bb = (size_t)im.F * sizeof(double4), cb = (size_t)im.P * 24, nb = (size_t)im.groups * 5 * sizeof(double);
    const size_t bytes = (im.bytes.size() + 255) / 256 * 256;
    HIPCHK(mem.alloc(&ms.faces, bytes + tail_bytes));
    unsigned char *blk = reinterpret_cast<unsigned char *>(ms.faces);
    const hipError_t e = hipMemcpy(blk, im.bytes.data(), im.bytes.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_clear(mem, ms); return hip_fail("guidance meshes: hipMemcpy", e); }
    ms.fbox = reinterpret_cast<double4 *>(blk + fb);
    ms.clouds = reinterpret_cast<double *>(blk + fb + bb);
    ms.bounds = reinterpret_cast<double *>(blk + fb + bb + cb);
    ms.ints = reinterpret_cast<int *>(blk + fb + bb + cb + nb);
    ms.groups = im.groups; ms.max_points = im.max_points; ms.mols = im.mols; ms.nfaces = im.F; ms.whole = im.whole;
    ms.grad_step = grad_step; ms.draws = d_draws;
    if (tail) *tail = blk + bytes;
    return 0;
}

// the per-step lists of mesh guidance for N atoms: [within N | outmesh N | counters 4 per group | unguided-step count 1 per
// group]; mesh_counters_clear zeroes the last two for a chain of n_groups
int mesh_workspace(shapemol_ctx *c, int64_t N, int64_t n_groups) {
    if (N <= c->m_cap && n_groups <= c->m_cnt_cap) return 0;
    N = std::max(N, c->m_cap); n_groups = std::max(n_groups, c->m_cnt_cap);
    c->drop_graphs();                            // the captured steps point into the old block
    HIPCHK(hipDeviceSynchronize());
    c->mem_mesh.release();
    c->m_out = c->m_cnt = nullptr; c->m_cap = c->m_cnt_cap = 0;
    HIPCHK(c->mem_mesh.alloc(&c->m_within, (size_t)N * 20 + (size_t)n_groups * 20));
    unsigned char *blk = reinterpret_cast<unsigned char *>(c->m_within);
    c->m_out = reinterpret_cast<int *>(blk + (size_t)N * 16);
    c->m_cnt = reinterpret_cast<int *>(blk + (size_t)N * 20);
    c->m_cap = N; c->m_cnt_cap = n_groups;
    return 0;
}
int mesh_counters_clear(shapemol_ctx *c, hipStream_t s, int64_t n_groups) {
    HIPCHK(hipMemsetAsync(c->m_cnt, 0, (size_t)n_groups * 4 * sizeof(int), s));
    HIPCHK(hipMemsetAsync(c->m_cnt + 4 * c->m_cnt_cap, 0, (size_t)n_groups * sizeof(int), s));
    c->m_flag_groups = n_groups;
    return 0;
}

// The launches of one kind of guidance on `pos` (Cfg and None: nothing here -- classifier-free guidance is part of the score
// evaluations and the posterior step).  In a chain step_cur is the device's step counter and t_first = T - 1; a stand-alone
// application passes no counter and t_first = grad_step + 1.
int enqueue_guidance(shapemol_ctx *c, hipStream_t s, Guide kind, float *pos, int64_t N, const int *step_cur, int t_first) {
    if (kind == Guide::Mesh) {               // each group of molecules against its own mesh
        const MeshGroupsArgs ma = mesh_args(c->ms, c->wg_table, c->m_within, c->m_out, c->m_cnt, c->m_cnt + 4 * c->m_cnt_cap, c->status,
                                            c->chain_params, pos, N, step_cur, t_first);
        const dim3 grid(groups_grid(N, c->ms.groups));
        LAUNCH("mesh_classify", SMK(mesh_classify_kernel, grid, dim3(256), mesh_lds_bytes(c->ms.max_points), s, ma));
        LAUNCH("mesh_pull", SMK(mesh_pull_kernel, grid, dim3(256), mesh_lds_bytes(c->ms.max_points), s, ma));
    } else if (kind == Guide::Cloud) {       // each group of molecules towards its own cloud
        const PcGroupsArgs ga = cloud_args(c->cs, c->wg_table, c->chain_params, pos, N, step_cur, t_first);
        LAUNCH("pc_guidance", SMK(pc_guidance_kernel, dim3(groups_grid(N, c->cs.groups)), dim3(256), cloud_lds_bytes(c->cs.max_points), s, ga));
    } else if (kind == Guide::Field) {       // each molecule down the gradient of its own shape's field (the chain's prep ran the prologue)
        int rc = 0;
        LAUNCH("field_guidance", rc = shapemol_sd_chain_guide_(c->field_sd, pos, c->mol_of, c->mol_off, N, c->lastB, c->field_lr, step_cur, t_first,
                                                                c->field_step, s, c->prof_on ? c->cur_e0 : nullptr, c->prof_on ? c->cur_e1 : nullptr));
        if (rc) return 1;
    }
    return 0;
}

// shapemol_guide_points*: one always-guided application of the context's guidance of `kind` to given positions
int guide_alone(shapemol_ctx *c, hipStream_t s, Guide kind, float *d_pos, int64_t N, const double *d_draws, uint64_t seed) {
    LAUNCH("prep", SMK(set_chain_params_kernel, dim3(1), dim3(1), 0, s, c->chain_params, guide_alone_params(seed, d_draws), c->steps));
    return enqueue_guidance(c, s, kind, d_pos, N, nullptr, (kind == Guide::Mesh ? c->ms.grad_step : c->cs.grad_step) + 1);
}

// shapemol_guide_points[_mesh] and their _groups siblings: the former have no batch vector and want a `whole` set
int guide_points_cloud(shapemol_ctx *c, const std::string &me, float *d_pos, const int64_t *d_batch, int64_t N, const double *d_draws,
                       uint64_t seed, void *stream) {
    if (!c || !d_pos || N < 1 || (d_batch && N > (1 << 27))) return fail(me + ": bad argument");
    if (c->cs.groups <= 0 || c->cs.whole != !d_batch)
        return fail(me + (d_batch ? ": no groups set (shapemol_set_guidance_groups)" : ": no cloud set (shapemol_set_guidance)"));
    HIPCHK(hipSetDevice(c->device));
    if (ensure_workspace(c, N, 1)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (c->cs.points == 0) return 0;             // no group has a cloud: nothing moves
    if (groups_table(c, s, d_batch, N, c->cs.ints, c->cs.groups)) return 1;
    return guide_alone(c, s, Guide::Cloud, d_pos, N, d_draws, seed);
}

int guide_points_mesh(shapemol_ctx *c, const std::string &me, float *d_pos, const int64_t *d_batch, int64_t N, const double *d_draws,
                      uint64_t seed, void *stream) {
    if (!c || !d_pos || N < 1 || N > (1 << 27)) return fail(me + ": bad argument");
    if (c->ms.groups <= 0 || c->ms.whole != !d_batch)
        return fail(me + (d_batch ? ": no groups set (shapemol_set_mesh_guidance_groups)" : ": no mesh set (shapemol_set_mesh_guidance)"));
    HIPCHK(hipSetDevice(c->device));
    if (ensure_workspace(c, N, 1) || mesh_workspace(c, N, c->ms.groups)) return 1;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(c->status + ST_MESH, 0, sizeof(int), s));
    if (c->ms.nfaces == 0) return 0;             // no group has a mesh: nothing moves
    if (mesh_counters_clear(c, s, c->ms.groups)) return 1;
    if (groups_table(c, s, d_batch, N, c->ms.ints, c->ms.groups)) return 1;
    return guide_alone(c, s, Guide::Mesh, d_pos, N, d_draws, seed);
}

}  // namespace

extern "C" {

int shapemol_set_guidance(shapemol_ctx *c, const double *h_cloud, int64_t n_points, double radius, int32_t grad_step, const double *d_draws) {
    if (!c) return fail("shapemol_set_guidance: null ctx");
    if (n_points < 0 || n_points > 2048 || (n_points > 0 && n_points < 3)) return fail("shapemol_set_guidance: the cloud needs 3 .. 2048 points (it is staged in LDS)");
    if (n_points > 0 && (!h_cloud || !(radius > 0.0))) return fail("shapemol_set_guidance: cloud / radius missing");
    HIPCHK(hipSetDevice(c->device));
    c->drop_graphs();                            // also drains the device: the old clouds may still be in use
    set_clear(c->mem_cs, c->cs);
    if (n_points == 0) return 0;
    return cloud_set_install_whole(c->mem_cs, c->cs, h_cloud, n_points, radius, grad_step, d_draws);
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
    set_clear(c->mem_cs, c->cs);
    if (n_groups == 0) return 0;
    return cloud_set_install(c->mem_cs, c->cs, n_groups, h_mol_off, h_clouds, h_cloud_off, h_radius, false, grad_step, d_draws);
}

int shapemol_guide_points_groups(shapemol_ctx *c, float *d_pos, const int64_t *d_batch, int64_t N, const double *d_draws, uint64_t seed,
                                 void *stream) {
    if (!d_batch) return fail("shapemol_guide_points_groups: bad argument");
    return guide_points_cloud(c, "shapemol_guide_points_groups", d_pos, d_batch, N, d_draws, seed, stream);
}

int shapemol_guide_points(shapemol_ctx *c, float *d_pos, int64_t N, const double *d_draws, uint64_t seed, void *stream) {
    return guide_points_cloud(c, "shapemol_guide_points", d_pos, nullptr, N, d_draws, seed, stream);
}

int shapemol_pointcloud_guidance(const double *h_cloud, int64_t n_points, double radius, double ratio, float *d_pos, int64_t N,
                                 const double *d_draws, uint64_t seed, void *stream) {
    if (!h_cloud || !d_pos || N < 1) return fail("shapemol_pointcloud_guidance: bad argument");
    if (n_points < 3 || n_points > 2048) return fail("shapemol_pointcloud_guidance: the cloud needs 3 .. 2048 points (it is staged in LDS)");
    if (!(radius > 0.0) || !(ratio >= 0.0 && ratio < 0.8)) return fail("shapemol_pointcloud_guidance: radius must be > 0, ratio in [0, 0.8)");
    hipStream_t s = (hipStream_t)stream;
    const unsigned n_wg = groups_grid(N, 1);
    const size_t o_step = (sizeof(ChainParams) + 15) / 16 * 16, o_table = o_step + 16;
    DevList mem; CloudSet cs;                           // a set of its own, and behind it [ChainParams | step counter | workgroup table]
    unsigned char *tail = nullptr;
    if (cloud_set_install_whole(mem, cs, h_cloud, n_points, radius, 0, nullptr, o_table + n_wg * sizeof(int2), &tail)) return 1;
    ChainParams *d_cp = reinterpret_cast<ChainParams *>(tail);
    int2 *d_table = reinterpret_cast<int2 *>(tail + o_table);
    hipLaunchKernelGGL(set_chain_params_kernel, dim3(1), dim3(1), 0, s, d_cp, guide_alone_params(seed, d_draws), reinterpret_cast<int *>(tail + o_step));
    hipLaunchKernelGGL(pc_groups_table_kernel, dim3(1), dim3(256), 0, s, (const int64_t *)nullptr, (int)N, cs.ints, cs.ints + 2, 1, cs.ints + 4,
                       cs.ints + 6, d_table, (int)n_wg);
    PcGroupsArgs ga = cloud_args(cs, d_table, d_cp, d_pos, N, nullptr, 1);      // t_first - 0 > grad_step = 0: always guided
    ga.ratio = ratio;
    hipLaunchKernelGGL(pc_guidance_kernel, dim3(n_wg), dim3(256), cloud_lds_bytes(n_points), s, ga);
    const hipError_t e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(s);       // the block is freed below; the reference's function is synchronous too
    set_clear(mem, cs);
    if (e != hipSuccess) return fail(std::string("shapemol_pointcloud_guidance: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(std::string("shapemol_pointcloud_guidance: ") + hipGetErrorString(e2));
    return 0;
}

int shapemol_set_field_guidance(shapemol_ctx *c, shapemol_sd_ctx *sd, double grad_lr, int32_t grad_step) {
    if (!c) return fail("shapemol_set_field_guidance: null ctx");
    if (sd) {
        int device = 0, latent = 0;
        shapemol_sd_describe_(sd, &device, &latent);
        if (device != c->device)
            return fail("shapemol_set_field_guidance: the decoder lives on device " + std::to_string(device) + ", the sampling context on device " + std::to_string(c->device));
        if (latent != c->cfg.shape_dim)
            return fail("shapemol_set_field_guidance: the decoder's latent is " + std::to_string(latent) + ", the model's shape_dim is " +
                        std::to_string(c->cfg.shape_dim) + ": a molecule is guided against the field of its own shape condition");
        if (!std::isfinite(grad_lr)) return fail("shapemol_set_field_guidance: grad_lr is not finite");
    }
    c->field_sd = sd; c->field_lr = sd ? grad_lr : 0.0; c->field_step = sd ? grad_step : 0;      // (part of the graph key: nothing to drop)
    return 0;
}

int shapemol_set_mesh_guidance(shapemol_ctx *c, const double *h_verts, int64_t n_verts, const int32_t *h_faces, int64_t n_faces,
                               const double *h_cloud, int64_t n_cloud, int32_t grad_step, const double *d_draws) {
    if (!c) return fail("shapemol_set_mesh_guidance: null ctx");
    if (n_faces < 0) return fail("shapemol_set_mesh_guidance: n_faces < 0");
    MeshSetImage img;
    if (n_faces > 0 && mesh_set_image_whole("shapemol_set_mesh_guidance", h_verts, n_verts, h_faces, n_faces, h_cloud, n_cloud, img)) return 1;
    HIPCHK(hipSetDevice(c->device));
    c->drop_graphs();                            // also drains the device: the old meshes may still be in use
    set_clear(c->mem_ms, c->ms);
    if (n_faces == 0) return 0;
    return mesh_set_install(c->mem_ms, c->ms, img, grad_step, d_draws);
}

int shapemol_guide_points_mesh(shapemol_ctx *c, float *d_pos, int64_t N, const double *d_draws, uint64_t seed, void *stream) {
    return guide_points_mesh(c, "shapemol_guide_points_mesh", d_pos, nullptr, N, d_draws, seed, stream);
}

int shapemol_set_mesh_guidance_groups(shapemol_ctx *c, int32_t n_groups, const int64_t *h_mol_off, const double *h_verts, const int64_t *h_vert_off,
                                      const int32_t *h_faces, const int64_t *h_face_off, const double *h_clouds, const int64_t *h_cloud_off,
                                      int32_t grad_step, const double *d_draws) {
    const std::string me = "shapemol_set_mesh_guidance_groups";
    if (!c) return fail(me + ": null ctx");
    if (n_groups < 0 || n_groups > (1 << 20)) return fail(me + ": n_groups out of range");
    MeshSetImage img;
    if (n_groups > 0 && mesh_set_image(me, false, n_groups, h_mol_off, h_verts, h_vert_off, h_faces, h_face_off, h_clouds, h_cloud_off, img)) return 1;
    HIPCHK(hipSetDevice(c->device));
    c->drop_graphs();                            // also drains the device: the old meshes may still be in use
    set_clear(c->mem_ms, c->ms);
    if (n_groups == 0) return 0;
    return mesh_set_install(c->mem_ms, c->ms, img, grad_step, d_draws);
}

int shapemol_guide_points_mesh_groups(shapemol_ctx *c, float *d_pos, const int64_t *d_batch, int64_t N, const double *d_draws, uint64_t seed,
                                      void *stream) {
    if (!d_batch) return fail("shapemol_guide_points_mesh_groups: bad argument");
    return guide_points_mesh(c, "shapemol_guide_points_mesh_groups", d_pos, d_batch, N, d_draws, seed, stream);
}

int shapemol_mesh_guidance(const double *h_verts, int64_t n_verts, const int32_t *h_faces, int64_t n_faces, const double *h_cloud,
                           int64_t n_cloud, float *d_pos, int64_t N, const double *d_draws, uint64_t seed, int32_t *flag_out,
                           void *stream) {
    if (flag_out) *flag_out = 0;
    if (!d_pos || N < 1 || N > (1 << 27)) return fail("shapemol_mesh_guidance: bad argument");
    MeshSetImage img;
    if (mesh_set_image_whole("shapemol_mesh_guidance", h_verts, n_verts, h_faces, n_faces, h_cloud, n_cloud, img)) return 1;
    hipStream_t s = (hipStream_t)stream;
    // a set of its own, and behind it [ChainParams | step counter, status [8], counters [4], unguided steps | table | within N | outmesh N]
    const unsigned n_wg = groups_grid(N, 1);
    const size_t o_misc = (sizeof(ChainParams) + 255) / 256 * 256, o_table = o_misc + 256;
    const size_t o_in = o_table + ((size_t)n_wg * sizeof(int2) + 255) / 256 * 256, o_out = o_in + (size_t)N * 16;
    DevList mem; MeshSet ms;
    unsigned char *tail = nullptr;
    if (mesh_set_install(mem, ms, img, 0, nullptr, o_out + (size_t)N * 4, &tail)) return 1;
    int *d_misc = reinterpret_cast<int *>(tail + o_misc);        // [0] step counter, [4 .. 11] status, [16 .. 19] counters, [20] unguided steps
    hipError_t e = hipMemsetAsync(d_misc, 0, 256, s);
    int32_t flag = 0;
    if (e == hipSuccess) {
        ChainParams *d_cp = reinterpret_cast<ChainParams *>(tail);
        int2 *d_table = reinterpret_cast<int2 *>(tail + o_table);
        hipLaunchKernelGGL(set_chain_params_kernel, dim3(1), dim3(1), 0, s, d_cp, guide_alone_params(seed, d_draws), d_misc);
        hipLaunchKernelGGL(pc_groups_table_kernel, dim3(1), dim3(256), 0, s, (const int64_t *)nullptr, (int)N, ms.ints, ms.ints + 2, 1, ms.ints + 4,
                           ms.ints + 6, d_table, (int)n_wg);
        const MeshGroupsArgs a = mesh_args(ms, d_table, reinterpret_cast<float4 *>(tail + o_in), reinterpret_cast<int *>(tail + o_out), d_misc + 16,
                                           d_misc + 20, d_misc + 4, d_cp, d_pos, N, nullptr, 1);      // t_first - 0 > grad_step = 0: always guided
        hipLaunchKernelGGL(mesh_classify_kernel, dim3(n_wg), dim3(256), mesh_lds_bytes((int)n_cloud), s, a);
        hipLaunchKernelGGL(mesh_pull_kernel, dim3(n_wg), dim3(256), mesh_lds_bytes((int)n_cloud), s, a);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_misc + 4 + ST_MESH, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    }
    const hipError_t e2 = hipStreamSynchronize(s);       // the block is freed below; the reference's function is synchronous too
    set_clear(mem, ms);
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
