// Mesh shape guidance with one mesh per GROUP of molecules (shapemol_set_mesh_guidance_groups).  A group is a contiguous run of
// molecules of the batch -- the batch vector is sorted, so also a contiguous run of atoms -- with its own mesh and cloud; a
// group without a mesh leaves its atoms alone.  One guided step is the single-mesh guidance of sm_mesh.h applied once per group
// to the group's atoms: the "within" atoms that anchor the pull and the 3-nearest search among them are PER GROUP.  Per atom
// the arithmetic is sm_mesh.h's own device functions (mesh_contains, mesh_cloud_d2, mesh_knn: fixed-ray parity with canonical
// edge order, float64 without FMA contraction, (squared distance, atom index) ordering), called on a per-group view of the
// concatenated data, so a list of one group gives the single-mesh kernels' bits.  Draws are keyed by the BATCH-GLOBAL atom
// (fed table [S][5][N] or Philox (atom, step, 200 + j)), as there.
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
// (n_within, n_outmesh) per group in the two alternating slots of sm_mesh.h (classify of step s adds into slot s & 1; the
// group's first pull workgroup clears the other slot).  All cleared before a chain starts.
//
// A group that fails the reference's KD-tree condition in a step (no within-atom, or fewer than 3 while an atom is to be
// pulled) raises ST_MESH and adds 1 to group_flags[g]: the number of steps in which group g was left unguided, for the error
// message of the chain (cleared with the counters).
//
// LDS: 24 B x the LARGEST cloud of the set, rounded up to 32 B so that the tile behind a group's cloud is aligned for its
// double4 / float4 accesses whatever the cloud's size, + the 16 KB tile; one dynamic size per launch (<= 64 KB: two workgroups =
// 8 waves per CU at the 2048-point limit, five at 512 points -- the single-mesh kernels' budget, now per group).
// ---------------------------------------------------------------------------------------------
#pragma once
#include "sm_mesh.h"

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

// the single-mesh argument block of group g: sm_mesh.h's device functions then see that group alone
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
SM_DEV int mesh_groups_tile_off(int n_points) { return (n_points * 3 + 3) & ~3; }
inline size_t mesh_groups_lds_bytes(int max_points) { return (((size_t)max_points * 3 + 3) & ~(size_t)3) * 8 + 16384; }

// 16 lanes per atom, 256 threads per block, blocks per the workgroup table
__global__ void __launch_bounds__(256) mesh_classify_groups_kernel(MeshGroupsArgs ga) {
    extern __shared__ double mesh_lds[];
    const int step = ga.step_cur ? *ga.step_cur : 0;
    if (ga.t_first - step <= ga.grad_step) return;                 // `if i > grad_step` (molopt_score_model.py:573)
    const int2 e = ga.wg_table[blockIdx.x];
    if (e.x < 0) return;
    const MeshGuideArgs a = mesh_group_view(ga, e.x);
    double *cloud = mesh_lds;
    double4 *tile = reinterpret_cast<double4 *>(mesh_lds + mesh_groups_tile_off(a.n_points));
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
// Reads only within-atoms and writes only outmesh atoms of the block's own group; the two sets are disjoint.
__global__ void __launch_bounds__(256) mesh_pull_groups_kernel(MeshGroupsArgs ga) {
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
    void *tile = mesh_lds + mesh_groups_tile_off(a.n_points);
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
                ph((uint32_t)atom, (uint32_t)step, (uint32_t)(200 + j), 0x3e5du, r);     // the single-mesh kernel's counter domain
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
