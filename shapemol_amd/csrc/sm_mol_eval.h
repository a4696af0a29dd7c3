// Geometry scores of sampled molecules: for every (frame, molecule) of a packed batch the bond order
// of every atom pair from distance thresholds (analyze.get_bond_order of the reference), the bonds per atom, the stable atoms,
// whether the molecule is stable, and per frame the C-C and all-pairs distance histograms (eval_bond_length.
// pair_distance_from_pos_v + get_pair_length_profile) and the class counts.  The rule -- thresholds, valences, bin edges,
// cut-offs, the class -> element table -- is data the caller passes; nothing of it is compiled in.
//
// Arithmetic: float64, in the reference's order, d = sqrt((dx*dx + dy*dy) + dz*dz) without contraction into FMAs (the pragma
// below), then the nested strict `<` tests on 100 * d.  d(i, j) and d(j, i) are the same bits (the differences are exact
// negations of each other), so each atom's owner sums its own bonds and nothing but the histograms needs an atomic; only
// pairs j > i feed the histograms.  A NaN distance fails every `<`: order 0, no histogram entry.  The bin of a distance is
// np.searchsorted(edges, d, side='left'), i.e. the number of edges < d, found by binary search over the edges in LDS.
//
// One kernel body, two launch forms (MevalPlan): a team of 64 threads (one wave) per (frame, molecule) for molecules of at
// most 64 atoms, four teams to the workgroup; a team of 256 threads (the workgroup) for molecules of up to 1024 atoms, thread t
// owning atoms t, t + 256, ...  A team stages its molecule in LDS as float64.  A workgroup stays inside one frame, keeps
// histograms and class counts in LDS as 32-bit counts and adds the non-zero ones to the frame's 64-bit counters when it ends.
// Only integers are accumulated, so every output is the same in every run.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#pragma clang fp contract(off)

constexpr int kMevalThreads = 256;                       // workgroup of both forms
constexpr int kMevalWaveAtoms = 64;                      // wave form: lane i owns atom i
constexpr int kMevalMaxAtoms = 1024;                     // block form: 25 KiB of LDS for the staged molecule
constexpr int kMevalMaxElements = 16;                    // 3 * 16 * 16 thresholds: 6 KiB of LDS
constexpr int kMevalMaxClasses = 32;
constexpr int kMevalMaxEdges = 255;                      // per histogram: 256 bins
constexpr int kMevalTargetBlocks = 8192;                 // workgroups of a launch once the frames alone do not fill the device
constexpr int64_t kMevalMaxMols = 1 << 20, kMevalMaxFrames = 1 << 20;
// iterations of one workgroup, so that its 32-bit LDS counts cannot wrap: 4 * 2016 pairs (wave), 523776 pairs (block) each
constexpr int kMevalMaxItersWave = 65536, kMevalMaxItersBlock = 2048;

struct MevalMol { int off, n; };                         // first atom and atom count of a molecule inside a frame

struct MevalArgs {
    const float *pos;                 // (F, N, 3)
    const void *cls;                  // (F, N) int32 or int64
    int cls64;
    long long N;                      // atoms per frame
    int F, B;
    const MevalMol *mol;              // (B)
    const int *jobs;                  // molecules of this launch form
    int n_jobs, gx, iters;            // workgroups per frame, and the job groups each of them loops over
    const double *thr;                // (3, E, E): bondsK + marginK
    const double *allowed;            // (E)
    const unsigned char *slot;        // (C) class -> element slot
    int E, C, carbon, hs;             // carbon: the slot of atomic number 6, or -1
    const double *cc_edges, *all_edges;
    int n_cc, n_all;
    double cc_cut, all_cut;
    int *nr_bonds;                    // (F, N)
    int *n_stable;                    // (F, B)
    unsigned char *mol_stable;        // (F, B)
    unsigned long long *hist_cc, *hist_all, *cls_counts;      // (F, n_cc + 1), (F, n_all + 1), (F, C), zero before the launch
    int *bad;                         // atoms whose class lies outside [0, C)
};

#if defined(__HIPCC__) && !defined(SM_MOL_EVAL_HOST_ONLY)

// number of edges < d: np.searchsorted(edges, d, side='left')
__device__ inline int meval_bin(const double *edges, int n, double d) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] < d) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <int TEAM>
__global__ __launch_bounds__(kMevalThreads) void meval_kernel(MevalArgs a) {
    constexpr int JPB = kMevalThreads / TEAM, CAP = TEAM == 64 ? kMevalWaveAtoms : kMevalMaxAtoms, OWN = CAP / TEAM;
    __shared__ double s_x[JPB * CAP], s_y[JPB * CAP], s_z[JPB * CAP];
    __shared__ double s_thr[3 * kMevalMaxElements * kMevalMaxElements], s_allowed[kMevalMaxElements];
    __shared__ double s_cc[kMevalMaxEdges + 1], s_all[kMevalMaxEdges + 1];
    __shared__ unsigned s_hcc[kMevalMaxEdges + 1], s_hall[kMevalMaxEdges + 1], s_cls[kMevalMaxClasses];
    __shared__ int s_stable[JPB];
    __shared__ unsigned char s_e[JPB * CAP], s_slot[kMevalMaxClasses];
    const int tid = threadIdx.x, team = tid / TEAM, lane = tid % TEAM;
    const int frame = blockIdx.x / a.gx, bx = blockIdx.x % a.gx;
    const int E = a.E, EE = a.E * a.E;
    for (int i = tid; i < 3 * EE; i += kMevalThreads) s_thr[i] = a.thr[i];
    for (int i = tid; i < E; i += kMevalThreads) s_allowed[i] = a.allowed[i];
    for (int i = tid; i < a.C; i += kMevalThreads) { s_slot[i] = a.slot[i]; s_cls[i] = 0; }
    for (int i = tid; i <= kMevalMaxEdges; i += kMevalThreads) {
        if (i < a.n_cc) s_cc[i] = a.cc_edges[i];
        if (i < a.n_all) s_all[i] = a.all_edges[i];
        s_hcc[i] = 0; s_hall[i] = 0;
    }
    double *x = s_x + team * CAP, *y = s_y + team * CAP, *z = s_z + team * CAP;
    unsigned char *el = s_e + team * CAP;
    for (int it = 0; it < a.iters; ++it) {
        const int job = (it * a.gx + bx) * JPB + team;
        const bool active = job < a.n_jobs;
        int m = 0, n = 0;
        size_t base = 0;
        if (active) { m = a.jobs[job]; n = a.mol[m].n; base = (size_t)frame * (size_t)a.N + (size_t)a.mol[m].off; }
        __syncthreads();                  // the tables are written; the iteration before has read its molecule
        if (lane == 0) s_stable[team] = 0;
        for (int i = lane; i < n; i += TEAM) {
            const float *p = a.pos + 3 * (base + i);
            x[i] = (double)p[0]; y[i] = (double)p[1]; z[i] = (double)p[2];
            const long long c = a.cls64 ? reinterpret_cast<const long long *>(a.cls)[base + i] : (long long)reinterpret_cast<const int *>(a.cls)[base + i];
            const bool ok = c >= 0 && c < a.C;
            el[i] = ok ? s_slot[c] : (unsigned char)0;
            if (ok) atomicAdd(&s_cls[c], 1u); else atomicAdd(a.bad, 1);
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
            const bool ci = ei == a.carbon;
            int sum = 0;
            for (int j = 0; j < n; ++j) {
                if (j == i) continue;
                const double dx = xi - x[j], dy = yi - y[j], dz = zi - z[j];
                const double d = sqrt((dx * dx + dy * dy) + dz * dz);
                const int ej = el[j];
                const double p = 100.0 * d;
                if (p < t1[ej]) sum += p < t2[ej] ? (p < t3[ej] ? 3 : 2) : 1;
                if (j > i) {
                    if (ci && ej == a.carbon && d < a.cc_cut) atomicAdd(&s_hcc[meval_bin(s_cc, a.n_cc, d)], 1u);
                    if (d < a.all_cut) atomicAdd(&s_hall[meval_bin(s_all, a.n_all, d)], 1u);
                }
            }
            a.nr_bonds[base + i] = sum;
            const double al = s_allowed[ei];
            stable += a.hs ? (al == (double)sum) : (al >= (double)sum && sum > 0);
        }
        if (stable) atomicAdd(&s_stable[team], stable);
        __syncthreads();
        if (active && lane == 0) {
            const size_t o = (size_t)frame * (size_t)a.B + (size_t)m;
            a.n_stable[o] = s_stable[team];
            a.mol_stable[o] = s_stable[team] == n;
        }
    }
    __syncthreads();
    for (int i = tid; i <= kMevalMaxEdges; i += kMevalThreads) {
        if (i <= a.n_cc && s_hcc[i]) atomicAdd(&a.hist_cc[(size_t)frame * (a.n_cc + 1) + i], (unsigned long long)s_hcc[i]);
        if (i <= a.n_all && s_hall[i]) atomicAdd(&a.hist_all[(size_t)frame * (a.n_all + 1) + i], (unsigned long long)s_hall[i]);
    }
    for (int i = tid; i < a.C; i += kMevalThreads)
        if (s_cls[i]) atomicAdd(&a.cls_counts[(size_t)frame * a.C + i], (unsigned long long)s_cls[i]);
}

#endif  // device code

// ---- host plan --------------------------------------------------------------------------------------------------------------
struct MevalForm { std::vector<int> jobs; int gx = 0, iters = 0; };      // the molecules of a launch form and its grid per frame

struct MevalPlan {
    std::vector<MevalMol> mol;
    MevalForm wave, block;
    std::vector<int> form;            // per molecule: 0 wave, 1 block
    long long N = 0;
};

// workgroups per frame and iterations per workgroup of a form with `jpb` jobs to the workgroup
inline void meval_form_grid(MevalForm &f, int jpb, int max_iters, int64_t F) {
    const int64_t groups = ((int64_t)f.jobs.size() + jpb - 1) / jpb;
    if (!groups) { f.gx = f.iters = 0; return; }
    int64_t gx = std::min<int64_t>(groups, std::max<int64_t>(1, (kMevalTargetBlocks + F - 1) / F));
    gx = std::max<int64_t>(gx, (groups + max_iters - 1) / max_iters);
    f.gx = (int)gx;
    f.iters = (int)((groups + gx - 1) / gx);
}

inline std::string meval_edges_error(const char *name, const double *edges, int n, double cut) {
    if (n < 1 || n > kMevalMaxEdges || !edges) return std::string("molecule evaluation: ") + name + " needs 1.." + std::to_string(kMevalMaxEdges) + " bin edges";
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(edges[i]) || (i && !(edges[i - 1] <= edges[i]))) return std::string("molecule evaluation: the ") + name + " bin edges must be finite and ascending";
    if (std::isnan(cut)) return std::string("molecule evaluation: the ") + name + " cut-off is NaN";
    return "";
}

// Checks a call and lays out its two launch forms.  "" or the refusal's message; `out` may be null.
inline std::string meval_plan(int64_t F, int64_t B, const int64_t *off, int E, int C, const int32_t *class_slot, const double *cc_edges, int n_cc,
                              double cc_cut, const double *all_edges, int n_all, double all_cut, MevalPlan *out) {
    if (F < 1 || F > kMevalMaxFrames) return "molecule evaluation: 1.." + std::to_string(kMevalMaxFrames) + " frames, got " + std::to_string(F);
    if (B < 1 || B > kMevalMaxMols || !off) return "molecule evaluation: 1.." + std::to_string(kMevalMaxMols) + " molecules, got " + std::to_string(B);
    if (E < 1 || E > kMevalMaxElements) return "molecule evaluation: the rule has " + std::to_string(E) + " elements; the limit is " + std::to_string(kMevalMaxElements);
    if (C < 1 || C > kMevalMaxClasses || !class_slot) return "molecule evaluation: " + std::to_string(C) + " atom classes; the limit is " + std::to_string(kMevalMaxClasses);
    for (int c = 0; c < C; ++c)
        if (class_slot[c] < 0 || class_slot[c] >= E) return "molecule evaluation: class " + std::to_string(c) + " has no element of the rule";
    std::string e = meval_edges_error("C-C", cc_edges, n_cc, cc_cut);
    if (e.empty()) e = meval_edges_error("all-pairs", all_edges, n_all, all_cut);
    if (!e.empty()) return e;
    if (off[0] != 0) return "molecule evaluation: the offsets must start at 0";
    MevalPlan pl;
    pl.mol.resize((size_t)B); pl.form.resize((size_t)B);
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = off[b + 1] - off[b];
        if (n < 1) return "molecule evaluation: molecule " + std::to_string(b) + " has no atoms";
        if (n > kMevalMaxAtoms) return "molecule evaluation: molecule " + std::to_string(b) + " has " + std::to_string(n) + " atoms; the limit is " + std::to_string(kMevalMaxAtoms);
        pl.mol[(size_t)b] = {(int)off[b], (int)n};
        const int form = n > kMevalWaveAtoms;
        pl.form[(size_t)b] = form;
        (form ? pl.block : pl.wave).jobs.push_back((int)b);
    }
    pl.N = off[B];
    meval_form_grid(pl.wave, kMevalThreads / 64, kMevalMaxItersWave, F);
    meval_form_grid(pl.block, 1, kMevalMaxItersBlock, F);
    if ((int64_t)pl.wave.gx * F >= (1ll << 31) || (int64_t)pl.block.gx * F >= (1ll << 31)) return "molecule evaluation: frames x molecules exceed one launch grid";
    if (out) *out = std::move(pl);
    return "";
}
