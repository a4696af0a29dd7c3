// The distance rule of sampled molecules, once, for the geometry scores (sm_mol_eval.h) and the bond
// graphs (sm_mol_graph.h, section 24): the limits, the argument blocks of a packed batch and of the rule, the device functions
// both kernels are made of up to and including the pair loop, and the host plan with its refusals.
//
// Arithmetic of a pair (mol_pair, the only place that has it): float64, in the reference's order,
// d = sqrt((dx*dx + dy*dy) + dz*dz) without contraction into FMAs (the pragma below), then the nested strict `<` tests on
// 100 * d.  d(i, j) and d(j, i) are the same bits (the differences are exact negations of each other).  A NaN distance fails
// every `<`: order 0, no histogram entry.  The bin of a distance is np.searchsorted(edges, d, side='left'), i.e. the number of
// edges < d, found by binary search over the edges in LDS.
//
// Frame of both kernels: two launch forms (MolPlan), a team of 64 threads (one wave) per (frame, molecule) for molecules of at
// most 64 atoms, four teams to the workgroup, or a team of 256 threads (the workgroup) for larger ones.  A team stages its
// molecule in LDS as float64.  A workgroup stays inside one frame, loops over job groups, keeps histograms and class counts in
// LDS as 32-bit counts and adds the non-zero ones to the frame's 64-bit counters when it ends.  The kernels declare the LDS
// arrays (a pass that needs none of a kind sizes it to 1) and hand them to the functions here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#pragma clang fp contract(off)

constexpr int kMolThreads = 256;                         // workgroup of both forms
constexpr int kMolWaveAtoms = 64;                        // wave form: lane i owns atom i
constexpr int kMolMaxElements = 16;                      // 3 * 16 * 16 thresholds: 6 KiB of LDS
constexpr int kMolMaxClasses = 32;
constexpr int kMolMaxEdges = 255;                        // per histogram: 256 bins
constexpr int kMolTargetBlocks = 8192;                   // workgroups of a launch once the frames alone do not fill the device
constexpr int64_t kMolMaxMols = 1 << 20, kMolMaxFrames = 1 << 20;
// iterations of one workgroup, so that its 32-bit LDS counts cannot wrap: per iteration at most 4 * 2016 pairs (wave) or 523776
// pairs (block, 1024 atoms) enter a histogram, 1024 atoms the class counts, 4 molecules any other counter
constexpr int kMolMaxItersWave = 65536, kMolMaxItersBlock = 2048;

struct MolSpan { int off, n; };                          // first atom and atom count of a molecule inside a frame

struct MolBatch {
    const float *pos;                 // (F, N, 3)
    const void *cls;                  // (F, N) int32 or int64
    int cls64;
    long long N;                      // atoms per frame
    int F, B;
    const MolSpan *mol;               // (B)
    const int *jobs;                  // molecules of this launch form
    int n_jobs, gx, iters;            // workgroups per frame, and the job groups each of them loops over
    int *bad;                         // atoms whose class lies outside [0, C)
};

struct MolRule {
    const double *thr;                // (3, E, E): bondsK + marginK
    const unsigned char *slot;        // (C) class -> element slot
    int E, C, carbon;                 // carbon: the slot of atomic number 6, or -1
    const double *cc_edges, *all_edges;
    int n_cc, n_all;
    double cc_cut, all_cut;
};

struct MolCounts { unsigned long long *hist_cc, *hist_all, *cls_counts; };      // (F, n_cc + 1), (F, n_all + 1), (F, C), zero before the launch

#if defined(__HIPCC__) && !defined(SM_MOL_EVAL_HOST_ONLY)

// number of edges < d: np.searchsorted(edges, d, side='left')
__device__ inline int mol_bin(const double *edges, int n, double d) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] < d) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// distance and bond order of a pair; t1, t2, t3: the rows of atom i's element in the three threshold tables
__device__ __forceinline__ int mol_pair(double xi, double yi, double zi, double xj, double yj, double zj, const double *t1, const double *t2,
                                        const double *t3, int ej, double &d) {
    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    d = sqrt((dx * dx + dy * dy) + dz * dz);
    const double p = 100.0 * d;
    int o = 0;
    if (p < t1[ej]) o = p < t2[ej] ? (p < t3[ej] ? 3 : 2) : 1;
    return o;
}

// the rule's tables into LDS and the class counts to zero; with `hist` the two sets of edges too, and their histograms to zero
__device__ __forceinline__ void mol_stage(const MolRule &r, bool hist, double *s_thr, unsigned char *s_slot, unsigned *s_cls, double *s_cc,
                                          double *s_all, unsigned *s_hcc, unsigned *s_hall) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 3 * r.E * r.E; i += kMolThreads) s_thr[i] = r.thr[i];
    for (int i = tid; i < r.C; i += kMolThreads) { s_slot[i] = r.slot[i]; s_cls[i] = 0; }
    if (!hist) return;
    for (int i = tid; i <= kMolMaxEdges; i += kMolThreads) {
        if (i < r.n_cc) s_cc[i] = r.cc_edges[i];
        if (i < r.n_all) s_all[i] = r.all_edges[i];
        s_hcc[i] = 0; s_hall[i] = 0;
    }
}

// the (frame, molecule) of a team in iteration `it` of workgroup bx of its frame, JPB teams to the workgroup
struct MolJob { bool active; int m, n, off; size_t base; };        // molecule, its atoms, its first atom in the frame and in the batch
template <int JPB> __device__ __forceinline__ MolJob mol_job(const MolBatch &b, int it, int bx, int team, int frame) {
    const int job = (it * b.gx + bx) * JPB + team;
    MolJob j{job < b.n_jobs, 0, 0, 0, 0};
    if (j.active) {
        j.m = b.jobs[job];
        j.n = b.mol[j.m].n; j.off = b.mol[j.m].off;
        j.base = (size_t)frame * (size_t)b.N + (size_t)j.off;
    }
    return j;
}

// atom i of the team's molecule (`at` in the batch) into LDS: the position as float64, the element slot of its class.  Returns
// the class, or -1 for one outside the table: the slot is 0 then and, with `flag`, the atom counts as bad
__device__ __forceinline__ int mol_load_atom(const MolBatch &b, const MolRule &r, size_t at, int i, bool flag, const unsigned char *s_slot, double *x,
                                             double *y, double *z, unsigned char *el) {
    const float *p = b.pos + 3 * at;
    x[i] = (double)p[0]; y[i] = (double)p[1]; z[i] = (double)p[2];
    const long long c = b.cls64 ? reinterpret_cast<const long long *>(b.cls)[at] : (long long)reinterpret_cast<const int *>(b.cls)[at];
    const bool ok = c >= 0 && c < r.C;
    el[i] = ok ? s_slot[c] : (unsigned char)0;
    if (!ok && flag) atomicAdd(b.bad, 1);
    return ok ? (int)c : -1;
}

// a pair j > i at distance d into the two LDS histograms; ci: atom i is a carbon
__device__ __forceinline__ void mol_hist_add(const MolRule &r, bool ci, int ej, double d, const double *s_cc, const double *s_all, unsigned *s_hcc,
                                             unsigned *s_hall) {
    if (ci && ej == r.carbon && d < r.cc_cut) atomicAdd(&s_hcc[mol_bin(s_cc, r.n_cc, d)], 1u);
    if (d < r.all_cut) atomicAdd(&s_hall[mol_bin(s_all, r.n_all, d)], 1u);
}

// the workgroup's non-zero LDS counts to the frame's 64-bit counters (behind a barrier after the last LDS add)
__device__ __forceinline__ void mol_flush(const MolRule &r, const MolCounts &o, int frame, const unsigned *s_hcc, const unsigned *s_hall,
                                          const unsigned *s_cls) {
    const int tid = threadIdx.x;
    for (int i = tid; i <= kMolMaxEdges; i += kMolThreads) {
        if (i <= r.n_cc && s_hcc[i]) atomicAdd(&o.hist_cc[(size_t)frame * (r.n_cc + 1) + i], (unsigned long long)s_hcc[i]);
        if (i <= r.n_all && s_hall[i]) atomicAdd(&o.hist_all[(size_t)frame * (r.n_all + 1) + i], (unsigned long long)s_hall[i]);
    }
    for (int i = tid; i < r.C; i += kMolThreads)
        if (s_cls[i]) atomicAdd(&o.cls_counts[(size_t)frame * r.C + i], (unsigned long long)s_cls[i]);
}

#endif  // device code

// ---- host plan --------------------------------------------------------------------------------------------------------------
struct MolForm { std::vector<int> jobs; int gx = 0, iters = 0; };        // the molecules of a launch form and its grid per frame

struct MolPlan {
    std::vector<MolSpan> mol;
    MolForm wave, block;
    std::vector<int> form;            // per molecule: 0 wave, 1 block
    long long N = 0;
};

// workgroups per frame and iterations per workgroup of a form with `jpb` jobs to the workgroup
inline void mol_form_grid(MolForm &f, int jpb, int max_iters, int64_t F) {
    const int64_t groups = ((int64_t)f.jobs.size() + jpb - 1) / jpb;
    if (!groups) { f.gx = f.iters = 0; return; }
    int64_t gx = std::min<int64_t>(groups, std::max<int64_t>(1, (kMolTargetBlocks + F - 1) / F));
    gx = std::max<int64_t>(gx, (groups + max_iters - 1) / max_iters);
    f.gx = (int)gx;
    f.iters = (int)((groups + gx - 1) / gx);
}

struct MolEdges { const char *name; const double *edges; int n; double cut; };      // the bin edges of one histogram of a call

inline std::string mol_edges_error(const std::string &what, const MolEdges &h) {
    if (h.n < 1 || h.n > kMolMaxEdges || !h.edges) return what + ": " + h.name + " needs 1.." + std::to_string(kMolMaxEdges) + " bin edges, got " + std::to_string(h.n);
    for (int i = 0; i < h.n; ++i)
        if (!std::isfinite(h.edges[i]) || (i && !(h.edges[i - 1] <= h.edges[i]))) return what + ": the " + h.name + " bin edges must be finite and ascending";
    if (std::isnan(h.cut)) return what + ": the " + h.name + " cut-off is NaN";
    return "";
}

// Checks a call of the feature `what` (the refusals' prefix) with its limit on a molecule's atoms and its histograms, and lays
// out the two launch forms.  "" or the refusal's message; `out` may be null.
inline std::string mol_plan(const std::string &what, int max_atoms, int64_t F, int64_t B, const int64_t *off, int E, int C, const int32_t *class_slot,
                            std::initializer_list<MolEdges> hists, MolPlan *out) {
    if (F < 1 || F > kMolMaxFrames) return what + ": 1.." + std::to_string(kMolMaxFrames) + " frames, got " + std::to_string(F);
    if (B < 1 || B > kMolMaxMols || !off) return what + ": 1.." + std::to_string(kMolMaxMols) + " molecules, got " + std::to_string(B);
    if (E < 1 || E > kMolMaxElements) return what + ": the rule has " + std::to_string(E) + " elements; the limit is " + std::to_string(kMolMaxElements);
    if (C < 1 || C > kMolMaxClasses || !class_slot) return what + ": " + std::to_string(C) + " atom classes; the limit is " + std::to_string(kMolMaxClasses);
    for (int c = 0; c < C; ++c)
        if (class_slot[c] < 0 || class_slot[c] >= E) return what + ": class " + std::to_string(c) + " has no element of the rule";
    for (const MolEdges &h : hists) {
        const std::string e = mol_edges_error(what, h);
        if (!e.empty()) return e;
    }
    if (off[0] != 0) return what + ": the offsets must start at 0";
    MolPlan pl;
    pl.mol.resize((size_t)B); pl.form.resize((size_t)B);
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = off[b + 1] - off[b];
        if (n < 1) return what + ": molecule " + std::to_string(b) + " has no atoms";
        if (n > max_atoms) return what + ": molecule " + std::to_string(b) + " has " + std::to_string(n) + " atoms; the limit is " + std::to_string(max_atoms);
        if (off[b + 1] >= (1ll << 31)) return what + ": molecule " + std::to_string(b) + " ends past 2^31 atoms in a frame";
        pl.mol[(size_t)b] = {(int)off[b], (int)n};
        const int form = n > kMolWaveAtoms;
        pl.form[(size_t)b] = form;
        (form ? pl.block : pl.wave).jobs.push_back((int)b);
    }
    pl.N = off[B];
    mol_form_grid(pl.wave, kMolThreads / kMolWaveAtoms, kMolMaxItersWave, F);
    mol_form_grid(pl.block, 1, kMolMaxItersBlock, F);
    if ((int64_t)pl.wave.gx * F >= (1ll << 31) || (int64_t)pl.block.gx * F >= (1ll << 31)) return what + ": frames x molecules exceed one launch grid";
    if (out) *out = std::move(pl);
    return "";
}
