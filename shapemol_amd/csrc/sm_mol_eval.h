// Geometry scores of sampled molecules: for every (frame, molecule) of a packed batch the bond order
// of every atom pair from distance thresholds (analyze.get_bond_order of the reference), the bonds per atom, the stable atoms,
// whether the molecule is stable, and per frame the C-C and all-pairs distance histograms (eval_bond_length.
// pair_distance_from_pos_v + get_pair_length_profile) and the class counts.  The rule -- thresholds, valences, bin edges,
// cut-offs, the class -> element table -- is data the caller passes; nothing of it is compiled in.
//
// The arithmetic of a pair, the two launch forms, the staging of a molecule, the LDS counters and the host plan are
// sm_mol_rule.h's, shared with the bond graphs (sm_mol_graph.h).  Each atom's owner sums the orders of its own pairs (d(i, j) and
// d(j, i) are the same bits), so nothing but the histograms needs an atomic; only pairs j > i feed the histograms.  This kernel
// takes molecules of up to 1024 atoms: in the block form thread t owns atoms t, t + 256, ...  Only integers are accumulated, so
// every output is the same in every run.
#pragma once
#include "sm_mol_rule.h"

#pragma clang fp contract(off)

constexpr int kMevalMaxAtoms = 1024;                     // block form: 25 KiB of LDS for the staged molecule

struct MevalArgs {
    MolBatch b;
    MolRule r;
    MolCounts o;
    const double *allowed;            // (E)
    int hs;
    int *nr_bonds;                    // (F, N)
    int *n_stable;                    // (F, B)
    unsigned char *mol_stable;        // (F, B)
};

#if defined(__HIPCC__) && !defined(SM_MOL_EVAL_HOST_ONLY)

template <int TEAM>
__global__ __launch_bounds__(kMolThreads) void meval_kernel(MevalArgs a) {
    constexpr int JPB = kMolThreads / TEAM, CAP = TEAM == 64 ? kMolWaveAtoms : kMevalMaxAtoms, OWN = CAP / TEAM;
    __shared__ double s_x[JPB * CAP], s_y[JPB * CAP], s_z[JPB * CAP];
    __shared__ double s_thr[3 * kMolMaxElements * kMolMaxElements], s_allowed[kMolMaxElements];
    __shared__ double s_cc[kMolMaxEdges + 1], s_all[kMolMaxEdges + 1];
    __shared__ unsigned s_hcc[kMolMaxEdges + 1], s_hall[kMolMaxEdges + 1], s_cls[kMolMaxClasses];
    __shared__ int s_stable[JPB];
    __shared__ unsigned char s_e[JPB * CAP], s_slot[kMolMaxClasses];
    const int tid = threadIdx.x, team = tid / TEAM, lane = tid % TEAM;
    const int frame = blockIdx.x / a.b.gx, bx = blockIdx.x % a.b.gx;
    const int E = a.r.E, EE = E * E;
    mol_stage(a.r, true, s_thr, s_slot, s_cls, s_cc, s_all, s_hcc, s_hall);
    for (int i = tid; i < E; i += kMolThreads) s_allowed[i] = a.allowed[i];
    double *x = s_x + team * CAP, *y = s_y + team * CAP, *z = s_z + team * CAP;
    unsigned char *el = s_e + team * CAP;
    for (int it = 0; it < a.b.iters; ++it) {
        const MolJob job = mol_job<JPB>(a.b, it, bx, team, frame);
        const int n = job.n;
        __syncthreads();                  // the tables are written; the iteration before has read its molecule
        if (lane == 0) s_stable[team] = 0;
        for (int i = lane; i < n; i += TEAM) {
            const int c = mol_load_atom(a.b, a.r, job.base + i, i, true, s_slot, x, y, z, el);
            if (c >= 0) atomicAdd(&s_cls[c], 1u);
        }
        __syncthreads();
        int stable = 0;
#pragma unroll
        for (int k = 0; k < OWN; ++k) {
            const int i = lane + k * TEAM;
            if (i >= n) continue;
            const double xi = x[i], yi = y[i], zi = z[i];
            const int ei = el[i];
            const double *t1 = s_thr + ei * E, *t2 = t1 + EE, *t3 = t2 + EE;
            const bool ci = ei == a.r.carbon;
            int sum = 0;
            for (int j = 0; j < n; ++j) {
                if (j == i) continue;
                double d;
                const int ej = el[j];
                sum += mol_pair(xi, yi, zi, x[j], y[j], z[j], t1, t2, t3, ej, d);
                if (j > i) mol_hist_add(a.r, ci, ej, d, s_cc, s_all, s_hcc, s_hall);
            }
            a.nr_bonds[job.base + i] = sum;
            const double al = s_allowed[ei];
            stable += a.hs ? (al == (double)sum) : (al >= (double)sum && sum > 0);
        }
        if (stable) atomicAdd(&s_stable[team], stable);
        __syncthreads();
        if (job.active && lane == 0) {
            const size_t o = (size_t)frame * (size_t)a.b.B + (size_t)job.m;
            a.n_stable[o] = s_stable[team];
            a.mol_stable[o] = s_stable[team] == n;
        }
    }
    __syncthreads();
    mol_flush(a.r, a.o, frame, s_hcc, s_hall, s_cls);
}

#endif  // device code

// the plan's types under the names they had while the scores were alone: host programs written against meval_plan keep compiling
using MevalForm = MolForm;
using MevalPlan = MolPlan;

// Checks a call and lays out its two launch forms.  "" or the refusal's message; `out` may be null.
inline std::string meval_plan(int64_t F, int64_t B, const int64_t *off, int E, int C, const int32_t *class_slot, const double *cc_edges, int n_cc,
                              double cc_cut, const double *all_edges, int n_all, double all_cut, MevalPlan *out) {
    return mol_plan("molecule evaluation", kMevalMaxAtoms, F, B, off, E, C, class_slot,
                    {{"C-C", cc_edges, n_cc, cc_cut}, {"all-pairs", all_edges, n_all, all_cut}}, out);
}
