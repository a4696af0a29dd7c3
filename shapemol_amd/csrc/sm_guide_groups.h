// Point-cloud shape guidance with one cloud per GROUP of molecules (shapemol_set_guidance_groups; shapemol_set_guidance is a set
// of one group that spans the batch).  A group is a contiguous run
// of molecules of the batch -- the batch vector is sorted, so also a contiguous run of atoms -- that shares one cloud and one
// radius; a group without a cloud leaves its atoms alone.  Per atom the work is pc_guide_atom of sm_misc.h, unchanged: 16 lanes
// per atom, float64 top-3 search with index tie-break, up to five pulls, float32 rounding at the end, draws keyed by the
// BATCH-GLOBAL atom index (fed table [S][5][N] or Philox (atom, step, 100 + j)).
//
// Mapping of workgroups to groups: a per-workgroup table, built on the device once per chain when the chain is enqueued
// (pc_groups_table_kernel; the molecules' atom ranges are known on the device only, from the batch vector).  Group g with n_g
// atoms and a cloud gets ceil(n_g / 16) workgroups of 256 threads (16 atoms x 16 lanes), numbered in group order; entry w holds
// (group, first atom).  A workgroup so serves atoms of one group only and stages that group's cloud.  The grid is the host-side
// bound floor(N / 16) + G, which the sum of the ceil(n_g / 16) cannot exceed; the table's unused tail is marked group = -1 and
// those workgroups return at once.  Grid, table address and LDS size depend on (N, G, largest cloud) only, never on the step, so
// the launch is captured in the chain's step graph; the `t > grad_step` gate reads the device step counter.
//
// LDS: one dynamic allocation per launch, 24 B x the LARGEST cloud of the chain (every workgroup of a launch gets the same
// size; it fills only its own group's 24 B x P_g).  With 512-point clouds that is 12 KB, and the 32-waves-per-CU cap (8
// workgroups of 4 waves) binds before the 160 KiB of LDS (13 workgroups); with one 2048-point cloud in the chain it is 48 KB,
// 3 workgroups = 12 waves per CU, for all groups of that chain.  The kernel is tens of microseconds of a step that takes 700
// and more (66 us at 5.5k atoms, 512 points, five pulls for every atom), so the simple uniform allocation is kept.
// The last workgroup of a group may be partly empty (< 16 atoms): at most 15 idle atom slots per group.
// ---------------------------------------------------------------------------------------------
#pragma once
#include "sm_misc.h"

struct PcGroupsArgs {
    float *pred_pos;          // [N][3] in/out
    const double *clouds;     // [sum P_g][3], the groups' clouds back to back
    const int *cloud_off;     // [G + 1] first point of each group's cloud (equal neighbours: no cloud)
    const double *radius;     // [G]
    const int *atom_off;      // [G + 1] first atom of each group (pc_groups_table_kernel)
    const int2 *wg_table;     // [gridDim.x] (group or -1, first atom of the workgroup)
    const ChainParams *cp;
    const int *step_cur;
    int n_atoms, t_first, grad_step;
    double ratio;
};

// One workgroup of 256 threads, once per chain.  mol_off[G + 1]: first molecule of each group (host-validated: starts at 0,
// does not decrease, ends at the number of molecules).  wg_off[G + 1] is scratch.  batch = nullptr: ONE group that spans
// whatever batch comes (the single-cloud / single-mesh entry points, which have no batch vector): its atoms are [0, n_atoms).
__global__ void __launch_bounds__(256) pc_groups_table_kernel(const int64_t *batch, int n_atoms, const int *mol_off, const int *cloud_off,
                                                              int n_groups, int *atom_off, int *wg_off, int2 *wg_table, int n_wg) {
    for (int g = threadIdx.x; g <= n_groups; g += blockDim.x) {      // first atom whose molecule is >= mol_off[g]
        if (!batch) { atom_off[g] = g ? n_atoms : 0; continue; }      // no batch vector: the one group is atoms [0, n_atoms)
        const int64_t m = mol_off[g];
        int lo = 0, hi = n_atoms;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (batch[mid] < m) lo = mid + 1; else hi = mid;
        }
        atom_off[g] = lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int w = 0;
        for (int g = 0; g < n_groups; ++g) {
            wg_off[g] = w;
            const int n_g = atom_off[g + 1] - atom_off[g];       // (negative only for an unsorted batch vector: no workgroup then)
            if (cloud_off[g + 1] > cloud_off[g] && n_g > 0) w += (n_g + 15) >> 4;
        }
        wg_off[n_groups] = w < n_wg ? w : n_wg;       // (w <= n_wg by construction; the clamp keeps every write inside the table)
    }
    __syncthreads();
    for (int g = threadIdx.x; g < n_groups; g += blockDim.x) {
        const int w1 = wg_off[g + 1] < wg_off[n_groups] ? wg_off[g + 1] : wg_off[n_groups];
        for (int w = wg_off[g]; w < w1; ++w) wg_table[w] = make_int2(g, atom_off[g] + ((w - wg_off[g]) << 4));
    }
    for (int w = wg_off[n_groups] + threadIdx.x; w < n_wg; w += blockDim.x) wg_table[w] = make_int2(-1, 0);
}

__global__ void __launch_bounds__(256) pc_guidance_kernel(PcGroupsArgs a) {
    extern __shared__ double pc_cloud[];                            // [largest P_g][3]; this workgroup fills [P_g][3]
    const int step = a.step_cur ? *a.step_cur : 0;
    if (a.t_first - step <= a.grad_step) return;                   // `if i > grad_step` (molopt_score_model.py:585)
    const int2 e = a.wg_table[blockIdx.x];
    if (e.x < 0) return;
    const int c0 = a.cloud_off[e.x], n_points = a.cloud_off[e.x + 1] - c0;
    const double *src = a.clouds + (size_t)c0 * 3;
    for (int i = threadIdx.x; i < n_points * 3; i += blockDim.x) pc_cloud[i] = src[i];
    __syncthreads();
    const int end = a.atom_off[e.x + 1];                            // > e.y: the table has no workgroup without an atom
    const int atom_raw = e.y + (threadIdx.x >> 4), l16 = threadIdx.x & 15;
    const int atom = atom_raw < end ? atom_raw : end - 1;
    pc_guide_atom(a.pred_pos, pc_cloud, n_points, a.radius[e.x], a.ratio, *a.cp, step, a.n_atoms, atom, atom_raw < end, l16);
}
