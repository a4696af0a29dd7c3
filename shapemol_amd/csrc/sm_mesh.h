// Mesh shape guidance (models/molopt_score_model.py:742-775, applied to the predicted x0 of the steps with t > grad_step,
// :571-580).  The reference runs it on the host (trimesh containment, sklearn KD-trees, numpy, one D2H + H2D round trip per
// step) with one mesh for the batch; here every GROUP of molecules has its own mesh and cloud (the reference's call is a set of
// one group that spans the batch), and a guided step is two kernels between the score evaluation and the posterior step:
//   mesh_classify_kernel  every atom: inside its group's mesh?  distance to the nearest cloud point?  -> per group, a compacted
//                         list of the "within" atoms (inside, > 0.4 from the cloud) and one of the "outmesh" atoms (outside, or
//                         inside but < 0.2 from the cloud).  The two sets are disjoint.
//   mesh_pull_kernel      the outmesh atoms only: up to five times, pull the atom away from the mean of its 3 nearest within-atoms
//                         (over the WHOLE group, as the reference's KD-tree of all within points) by u * 0.8 + 0.2, and accept
//                         the moved point when it is inside the mesh and > 0.2 from the cloud.  Atoms never accepted keep their
//                         original position (the reference writes only the accepted ones).
// Precision as numpy's on the float32 prediction: the mean of the three within-atoms is float32 ((a + b) + c) / 3 in ascending
// distance order; the pull direction is float32 in the first iteration (float32 - float32), float64 from the second on; the
// moved points, distances and neighbour searches are float64; the result is rounded to float32.  Products are never
// contracted into FMAs here (numpy and the host code do not), so the arithmetic is the same as tests/mesh_oracle.py's.
//
// Containment: parity of the crossings of one fixed ray.  Every point is mapped by the fixed orthonormal matrix kMeshRot
// (rows r0 = (0.8, -0.6, 0), r1 = (0.36, 0.48, -0.8), r2 = r0 x r1 = (0.48, 0.64, 0.6)) to (u, v, w) = (r0.x, r1.x, r2.x); the
// ray runs along +w, i.e. along (0.48, 0.64, 0.6) in model space (up to the rounding of the constants, which only tilts the
// one ray every point uses).  A face is crossed when the projected point lies in the projected triangle and the hit lies at a
// larger w.  The three edge functions are evaluated with each edge's endpoints in canonical order (lower vertex index first),
// so the two faces sharing an edge compute the same value and see it with opposite signs; a zero counts as positive in the
// canonical orientation, so a ray through a shared edge counts exactly one of the two faces.  Vertices are projected once on
// the host (the same operations in the same order), faces carry their projected bounding box for the early-out.
// ---------------------------------------------------------------------------------------------
#pragma once
#include "sm_misc.h"

constexpr double kMeshRot[3][3] = {{0.8, -0.6, 0.0}, {0.36, 0.48, -0.8}, {0.48, 0.64, 0.6}};
constexpr int kMeshFaceTile = 512;        // face boxes per LDS tile (32 B each: 16 KB)
constexpr int kMeshWithinTile = 1024;     // within-atoms per LDS tile (float4 each: 16 KB); the cloud takes <= 48 KB beside

struct MeshFace {                         // projected vertices of one face in its own order (A, B, C)
    double u[3], v[3], w[3];
    int canon;                            // bit k: edge k (AB, BC, CA) runs from the lower vertex index to the higher
    int pad;
};

struct MeshGuideArgs {
    float *pred_pos;                      // [N][3] in/out
    const double *cloud;                  // [P][3]
    const MeshFace *faces;                // [F]
    const double4 *fbox;                  // [F] (umin, umax, vmin, vmax) of every projected face
    float4 *within;                       // [N] compacted within-atoms: x, y, z, atom index (bits)
    int *out_list;                        // [N] compacted outmesh atoms
    int *cnt;                             // [2][2] (n_within, n_outmesh), slot (step & 1); see mesh_pull_kernel
    int *status;                          // ST_MESH is raised here
    const ChainParams *cp;
    const int *step_cur;
    int n_atoms, n_points, n_faces, t_first, grad_step;
    double umin, umax, vmin, vmax, wmax;  // bounds of the projected mesh (the early-out before the face scan)
};

__host__ __device__ inline void mesh_project(double x, double y, double z, double &u, double &v, double &w) {
#pragma clang fp contract(off)
    u = (kMeshRot[0][0] * x + kMeshRot[0][1] * y) + kMeshRot[0][2] * z;
    v = (kMeshRot[1][0] * x + kMeshRot[1][1] * y) + kMeshRot[1][2] * z;
    w = (kMeshRot[2][0] * x + kMeshRot[2][1] * y) + kMeshRot[2][2] * z;
}

// 1 if the ray from (qu, qv, qw) along +w crosses face f
SM_DEV int mesh_face_cross(const MeshFace &f, double qu, double qv, double qw) {
#pragma clang fp contract(off)
    double e[3];
    bool pos[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = k, b = k == 2 ? 0 : k + 1;
        const bool cn = (f.canon >> k) & 1;
        const int lo = cn ? a : b, hi = cn ? b : a;
        const double ec = (f.u[hi] - f.u[lo]) * (qv - f.v[lo]) - (f.v[hi] - f.v[lo]) * (qu - f.u[lo]);
        const bool p = ec >= 0.0;                        // zero: positive in the canonical orientation
        pos[k] = cn ? p : !p;                            // sign seen in the face's own orientation
        e[k] = cn ? ec : -ec;
    }
    if (pos[0] != pos[1] || pos[1] != pos[2]) return 0;
    // hit depth relative to q, times the (signed) doubled projected area: e_BC (wA - q) + e_CA (wB - q) + e_AB (wC - q)
    const double d = (e[1] * (f.w[0] - qw) + e[2] * (f.w[1] - qw)) + e[0] * (f.w[2] - qw);
    return pos[0] ? (d > 0.0) : (d < 0.0);
}

SM_DEV double mesh_min_f64(double v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v = fmin(v, shfl_xor_f64(v, m));
    return v;
}

// squared distance of p to the nearest cloud point (cloud in LDS), identical in the 16 lanes of the atom
SM_DEV double mesh_cloud_d2(const double *cloud, int n_points, const double (&p)[3], int l16) {
#pragma clang fp contract(off)
    double best = 1e300;
    for (int c = l16; c < n_points; c += 16) {
        const double dx = p[0] - cloud[c * 3], dy = p[1] - cloud[c * 3 + 1], dz = p[2] - cloud[c * 3 + 2];
        best = fmin(best, (dx * dx + dy * dy) + dz * dz);
    }
    return mesh_min_f64(best);
}

// containment of p (the atom's 16 lanes agree); block-uniform control flow: every thread of the block calls it, `live`
// lanes do the work.  The face boxes stream through LDS (tile: kMeshFaceTile), a face's vertices are read from global
// memory only when the projected point lies in its box.
SM_DEV bool mesh_contains(const MeshGuideArgs &a, double4 *tile, const double (&p)[3], bool live, int l16) {
    double qu, qv, qw;
    mesh_project(p[0], p[1], p[2], qu, qv, qw);
    live = live && qu >= a.umin && qu <= a.umax && qv >= a.vmin && qv <= a.vmax && qw <= a.wmax;   // the ray misses the mesh
    int par = 0;
    if (__syncthreads_or(live)) {
        for (int f0 = 0; f0 < a.n_faces; f0 += kMeshFaceTile) {
            const int nt = min(kMeshFaceTile, a.n_faces - f0);
            __syncthreads();
            for (int i = threadIdx.x; i < nt; i += blockDim.x) tile[i] = a.fbox[f0 + i];
            __syncthreads();
            if (live) {
                for (int f = l16; f < nt; f += 16) {
                    const double4 b = tile[f];
                    if (qu >= b.x && qu <= b.y && qv >= b.z && qv <= b.w) par ^= mesh_face_cross(a.faces[f0 + f], qu, qv, qw);
                }
            }
        }
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) par ^= __shfl_xor(par, m, 64);
    return par != 0;
}

SM_DEV void mesh_load_cloud(const MeshGuideArgs &a, double *cloud) {
    for (int i = threadIdx.x; i < a.n_points * 3; i += blockDim.x) cloud[i] = a.cloud[i];
    __syncthreads();
}

// Three nearest within-atoms of p (key: squared distance, then atom index), identical in the atom's 16 lanes.  Block-uniform.
SM_DEV Top3 mesh_knn(const MeshGuideArgs &a, float4 *tile, int n_within, const double (&p)[3], bool live, int l16) {
#pragma clang fp contract(off)
    Top3 t{{1e300, 1e300, 1e300}, {0x7ffffff0, 0x7ffffff1, 0x7ffffff2}};
    for (int w0 = 0; w0 < n_within; w0 += kMeshWithinTile) {
        const int nt = min(kMeshWithinTile, n_within - w0);
        __syncthreads();
        for (int i = threadIdx.x; i < nt; i += blockDim.x) tile[i] = a.within[w0 + i];
        __syncthreads();
        if (live) {
            for (int c = l16; c < nt; c += 16) {
                const float4 q = tile[c];
                const double dx = p[0] - (double)q.x, dy = p[1] - (double)q.y, dz = p[2] - (double)q.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (__any(key_less(d2, __float_as_int(q.w), t.d[2], t.i[2]))) top3_insert(t, d2, __float_as_int(q.w));
            }
        }
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
        Top3 o;
#pragma unroll
        for (int k = 0; k < 3; ++k) { o.d[k] = shfl_xor_f64(t.d[k], m); o.i[k] = __shfl_xor(t.i[k], m, 64); }
#pragma unroll
        for (int k = 0; k < 3; ++k) top3_insert(t, o.d[k], o.i[k]);
    }
    return t;
}

// ---- the kernels.  A group is a contiguous run of molecules of the batch -- the batch vector is sorted, so also a contiguous
// run of atoms -- with its own mesh and cloud; a group without a mesh leaves its atoms alone.  Per atom the arithmetic is the
// device functions above, called on a per-group view of the concatenated data (mesh_group_view).  Draws are keyed by the
// BATCH-GLOBAL atom (fed table [S][5][N] or Philox (atom, step, 200 + j)).
//
// Device data, one block per installed set: faces, face boxes and clouds of all groups back to back with CSR offsets per group
// (face_off, cloud_off), and the projected bounds [G][5] of every mesh.
//
// Mapping of workgroups to groups: the per-workgroup table of sm_guide_groups.h (pc_groups_table_kernel, once per chain):
// group g with n_g atoms and a mesh gets ceil(n_g / 16) workgroups of 256 threads (16 atoms x 16 lanes); entry w holds
// (group, first atom); the unused tail of the grid floor(N / 16) + G is marked -1 and returns at once, as do the workgroups of
// groups without a mesh (they have none).  A workgroup stages only its group's cloud and streams only its group's face boxes /
// within-atoms through the 16 KB tile.  Both kernels use the same table: in the pull kernel the workgroup whose first atom is
// atom_off[g] + 16 i serves the outmesh slots [16 i, 16 i + 16) of group g and returns when the group has fewer.
//
// Per-step lists: within [N] and outmesh [N] are segmented by the groups' atom ranges (group g compacts into
// [atom_off[g], atom_off[g + 1]): it cannot have more within- or outmesh atoms than atoms); counters [G][2][2] =
// (n_within, n_outmesh) per group in two alternating slots: classify of step s adds into slot (s & 1); pull of step s reads that
// slot, and the group's first pull workgroup clears slot ((s + 1) & 1), which the previous step used and the next step's classify
// fills.  All cleared before a chain starts.
//
// A group that fails the reference's KD-tree condition in a step (no within-atom, or fewer than 3 while an atom is to be
// pulled) raises ST_MESH and adds 1 to group_flags[g]: the number of steps in which group g was left unguided, for the error
// message of the chain (cleared with the counters).
//
// LDS: 24 B x the LARGEST cloud of the set, rounded up to 32 B so that the tile behind a group's cloud is aligned for its
// double4 / float4 accesses whatever the cloud's size, + the 16 KB tile; one dynamic size per launch (<= 64 KB: two workgroups =
// 8 waves per CU at the 2048-point limit, five at 512 points).
struct MeshGroupsArgs {
    float *pred_pos;              // [N][3] in/out
    const double *clouds;         // [sum P_g][3]
    const MeshFace *faces;        // [sum F_g]
    const double4 *fbox;          // [sum F_g]
    const double *bounds;         // [G][5] (umin, umax, vmin, vmax, wmax) of every projected mesh
    const int *face_off;          // [G + 1]
    const int *cloud_off;         // [G + 1] (equal neighbours: no mesh)
    const int *atom_off;          // [G + 1] first atom of each group (pc_groups_table_kernel)
    const int2 *wg_table;         // [gridDim.x] (group or -1, first atom of the workgroup)
    float4 *within;               // [N], segment of group g at atom_off[g]
    int *out_list;                // [N], likewise
    int *cnt;                     // [G][2][2]
    int *group_flags;             // [G] steps in which the group was left unguided (too few within-atoms)
    int *status;
    const ChainParams *cp;
    const int *step_cur;
    int n_atoms, t_first, grad_step;
};

// the argument block of group g: the device functions above then see that group alone
SM_DEV MeshGuideArgs mesh_group_view(const MeshGroupsArgs &a, int g) {
    MeshGuideArgs v;
    const int f0 = a.face_off[g], c0 = a.cloud_off[g], a0 = a.atom_off[g];
    v.pred_pos = a.pred_pos; v.cloud = a.clouds + (size_t)c0 * 3; v.faces = a.faces + f0; v.fbox = a.fbox + f0;
    v.within = a.within + a0; v.out_list = a.out_list + a0; v.cnt = a.cnt + 4 * g; v.status = a.status; v.cp = a.cp;
    v.step_cur = a.step_cur; v.n_atoms = a.n_atoms; v.n_points = a.cloud_off[g + 1] - c0; v.n_faces = a.face_off[g + 1] - f0;
    v.t_first = a.t_first; v.grad_step = a.grad_step;
    const double *b = a.bounds + 5 * g;
    v.umin = b[0]; v.umax = b[1]; v.vmin = b[2]; v.vmax = b[3]; v.wmax = b[4];
    return v;
}

// doubles of LDS in front of the tile: the group's cloud, rounded up to a multiple of 32 bytes
SM_DEV int mesh_tile_off(int n_points) { return (n_points * 3 + 3) & ~3; }
inline size_t mesh_lds_bytes(int max_points) { return (((size_t)max_points * 3 + 3) & ~(size_t)3) * 8 + 16384; }

// 16 lanes per atom, 256 threads per block, blocks per the workgroup table
__global__ void __launch_bounds__(256) mesh_classify_kernel(MeshGroupsArgs ga) {
    extern __shared__ double mesh_lds[];
    const int step = ga.step_cur ? *ga.step_cur : 0;
    if (ga.t_first - step <= ga.grad_step) return;                 // `if i > grad_step` (molopt_score_model.py:573)
    const int2 e = ga.wg_table[blockIdx.x];
    if (e.x < 0) return;
    const MeshGuideArgs a = mesh_group_view(ga, e.x);
    double *cloud = mesh_lds;
    double4 *tile = reinterpret_cast<double4 *>(mesh_lds + mesh_tile_off(a.n_points));
    mesh_load_cloud(a, cloud);
    const int end = ga.atom_off[e.x + 1];                          // > e.y: the table has no workgroup without an atom
    const int atom_raw = e.y + (threadIdx.x >> 4), l16 = threadIdx.x & 15;
    const bool ok = atom_raw < end;
    const int atom = ok ? atom_raw : end - 1;
    const float x = a.pred_pos[atom * 3], y = a.pred_pos[atom * 3 + 1], z = a.pred_pos[atom * 3 + 2];
    const double p[3] = {(double)x, (double)y, (double)z};
    const double d = sqrt(mesh_cloud_d2(cloud, a.n_points, p, l16));
    const bool inside = mesh_contains(a, tile, p, ok, l16);
    if (ok && l16 == 0) {
        int *cnt = a.cnt + 2 * (step & 1);
        if (inside && d > 0.4) a.within[atomicAdd(cnt, 1)] = make_float4(x, y, z, __int_as_float(atom));
        else if (!inside || d < 0.2) a.out_list[atomicAdd(cnt + 1, 1)] = atom;
    }
}

// One block per 16 outmesh slots of a group (the table gives every group as many blocks as it could have outmesh atoms).
// Reads only within-atoms (their positions: the compacted copy and, by index, pred_pos) and writes only outmesh atoms of the
// block's own group, and the two sets are disjoint: updating pred_pos in place is race-free.
__global__ void __launch_bounds__(256) mesh_pull_kernel(MeshGroupsArgs ga) {
#pragma clang fp contract(off)
    extern __shared__ double mesh_lds[];
    const int step = ga.step_cur ? *ga.step_cur : 0;
    const int2 e = ga.wg_table[blockIdx.x];
    if (e.x < 0) return;
    const int base = e.y - ga.atom_off[e.x];                       // first outmesh slot of this block within its group
    int *gcnt = ga.cnt + 4 * e.x;
    if (base == 0 && threadIdx.x < 2) gcnt[2 * ((step + 1) & 1) + threadIdx.x] = 0;
    if (ga.t_first - step <= ga.grad_step) return;
    const int n_within = gcnt[2 * (step & 1)], n_out = gcnt[2 * (step & 1) + 1];
    if (n_within == 0 || (n_within < 3 && n_out > 0)) {          // the reference's KDTree(...) / query(k=3) raise ValueError
        if (base == 0 && threadIdx.x == 0) { ga.status[ST_MESH] = 1; atomicAdd(ga.group_flags + e.x, 1); }
        return;
    }
    if (base >= n_out) return;
    const MeshGuideArgs a = mesh_group_view(ga, e.x);
    double *cloud = mesh_lds;
    void *tile = mesh_lds + mesh_tile_off(a.n_points);
    mesh_load_cloud(a, cloud);
    const int slot = base + (threadIdx.x >> 4), l16 = threadIdx.x & 15;
    const bool ok = slot < n_out;
    const int atom = a.out_list[ok ? slot : base];
    const float p32[3] = {a.pred_pos[atom * 3], a.pred_pos[atom * 3 + 1], a.pred_pos[atom * 3 + 2]};
    double p[3] = {(double)p32[0], (double)p32[1], (double)p32[2]};
    bool live = ok, accepted = false;
    const ChainParams cp = *a.cp;
    for (int j = 0; j < 5; ++j) {
        if (!__syncthreads_or(live)) break;
        const Top3 t = mesh_knn(a, reinterpret_cast<float4 *>(tile), n_within, p, live, l16);
        if (live) {
            double u;
            if (cp.guide_draws) {
                u = cp.guide_draws[((size_t)(step - cp.step_base) * 5 + j) * a.n_atoms + atom];
            } else {
                Philox ph{(uint32_t)cp.seed, (uint32_t)(cp.seed >> 32)};
                uint32_t r[4];
                ph((uint32_t)atom, (uint32_t)step, (uint32_t)(200 + j), 0x3e5du, r);     // the point-cloud kernel uses 100 + j
                u = ((double)(r[0] >> 5) * 67108864.0 + (double)(r[1] >> 6)) * (1.0 / 9007199254740992.0);
            }
            const double scalar = u * 0.8 + 0.2;                  // np.random.random() * 0.8 + 0.2
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float mean = ((a.pred_pos[t.i[0] * 3 + k] + a.pred_pos[t.i[1] * 3 + k]) + a.pred_pos[t.i[2] * 3 + k]) / 3.0f;
                const double dir = j == 0 ? (double)(p32[k] - mean) : p[k] - (double)mean;
                p[k] = p[k] - scalar * dir;
            }
        }
        const bool inside = mesh_contains(a, reinterpret_cast<double4 *>(tile), p, live, l16);
        const double d = sqrt(mesh_cloud_d2(cloud, a.n_points, p, l16));
        if (live && inside && d > 0.2) { accepted = true; live = false; }
    }
    if (accepted && l16 < 3) a.pred_pos[atom * 3 + l16] = (float)(l16 == 0 ? p[0] : (l16 == 1 ? p[1] : p[2]));
}
