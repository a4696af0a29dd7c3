// Bond graphs of sampled molecules: for every (frame, molecule) of a packed batch the bonds that the
// distance rule of sm_mol_rule.h finds (meval_kernel of sm_mol_eval.h keeps only their sum per atom), with their orders, the
// fragments, whether the molecule is complete (one fragment), the shortest cycle through every bond, and per frame the
// bond-length histograms, the pair-distance histograms and class counts of the complete molecules, and how many molecules are
// complete or hold a ring of each size.  The rule is this project's own -- the caller's thresholds -- not a chemistry toolkit's
// bond perception.
//
// Arithmetic of a pair: mol_pair of sm_mol_rule.h, the function meval_kernel's pair loop calls, so an atom's orders add up to
// meval_kernel's nr_bonds bit for bit.  Everything after it is integer work on bit masks.
//
// One kernel body, two launch forms (MolPlan): a team of 64 threads (one wave) per (frame, molecule) for molecules of at most
// 64 atoms, four teams to the workgroup; a team of 256 threads (the workgroup) for molecules of 65..256 atoms.  Thread i of a
// team owns atom i.  A team keeps the adjacency of its molecule in LDS as bit masks, W = 1 or 4 64-bit words per atom: thread i
// forms row i in registers from its own pair loop (d(i, j) and d(j, i) are the same bits, so the matrix is symmetric without
// any exchange) and stores it.  Orders are not stored: the few places that need one (the owner of a bond when it writes the
// bond) recompute the pair.  Two passes over the same body: pass 0 counts the bonds of every (frame, molecule), a scan kernel
// turns the counts into offsets, pass 1 recomputes the rows and writes everything.  A bond (i, j), i < j, is written by thread i
// at offset[frame, molecule] + (bonds of atoms < i to higher atoms) + (its rank among i's higher neighbours): frame, molecule,
// (i, j) order with no atomic.
//
// Every loop whose trip count depends on the data is left through __syncthreads_or, so all barriers are reached by the whole
// workgroup in both forms.  Histograms and counters of a frame: 32-bit LDS counts added to the frame's 64-bit counters when the
// workgroup ends, sm_mol_rule.h's scheme with its bound on iterations per workgroup -- except the bond-length histograms, whose
// table (pairs of elements x 3 orders x bins, up to 136 x 3 x 256 counts) does not fit LDS: a bond adds 1 to its 64-bit global
// counter directly, about one atomic per atom against the pair loop's n / 2 distances.  Only integers are added, so every output
// is the same in every run.
#pragma once
#include "sm_mol_rule.h"

#pragma clang fp contract(off)

constexpr int kMgraphMaxAtoms = 256;                     // one atom per thread; block form: four mask words per atom (8 KiB)
constexpr int kMgraphRingBits = 32;                      // ring_sizes: bit s for a ring of s bonds, 3 <= s <= 30; bit 31: larger
constexpr int kMgraphScanItems = 8;                      // consecutive counts per thread of the scan kernel

struct MgraphArgs {
    MolBatch b;
    MolRule r;
    MolCounts o;                      // of the complete molecules
    const double *bl_edges;
    int n_bl;
    int *count;                       // (F * B) bonds per (frame, molecule): pass 0 writes, the scan reads
    const long long *offset;          // (F * B + 1): pass 1 reads
    int *nr_bonds, *degree, *frag, *ring_atom;                               // (F, N)
    int *mol_out;                     // (F, B, 6): bonds, fragments, largest fragment, complete, cycles, ring_sizes
    int *bonds;                       // (total, 3)
    int *ring_bond;                   // (total)
    unsigned long long *hist_bl;      // (F, 2, E (E + 1) / 2, 3, n_bl + 1): all molecules | complete ones
    unsigned long long *frame_counts; // (F, 1 + kMgraphRingBits): complete molecules, then molecules with a ring of bit s
};

#if defined(__HIPCC__) && !defined(SM_MOL_EVAL_HOST_ONLY)

struct MgSum { __device__ int operator()(int a, int b) const { return a + b; } };
struct MgMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct MgOr { __device__ int operator()(int a, int b) const { return a | b; } };

// op over the team's values, the result in every thread.  Block form: s_w (4) holds the waves' results between two barriers
template <int TEAM, typename Op> __device__ __forceinline__ int mg_reduce(int v, Op op, int *s_w) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    if (TEAM == 64) return v;
    __syncthreads();                      // s_w may still be read from a call before
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(s_w[0], s_w[1]), op(s_w[2], s_w[3]));
}

// exclusive prefix sum over the team's threads
template <int TEAM> __device__ __forceinline__ int mg_scan(int v, int *s_w) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (TEAM == 64) return inc - v;
    __syncthreads();
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (i < w) base += s_w[i];
    return base + inc - v;
}

// bits of word w of a row that name atoms above i
template <int W> __device__ __forceinline__ unsigned long long mg_above(unsigned long long word, int w, int i) {
    const int iw = i >> 6;
    if (w < iw) return 0ull;
    if (w > iw) return word;
    return (i & 63) == 63 ? 0ull : word & (~0ull << ((i & 63) + 1));
}

// Bonds in the shortest cycle through bond (i, j): 1 + the distance from i to j in the graph without that bond, level by
// level over the adjacency masks with the frontier as a mask; 0 when j cannot be reached (a bridge)
template <int W> __device__ __forceinline__ int mg_ring(const unsigned long long *adj, int i, int j) {
    unsigned long long vis[W], fr[W];
    const int jw = j >> 6;
    const unsigned long long jbit = 1ull << (j & 63);
#pragma unroll
    for (int w = 0; w < W; ++w) vis[w] = fr[w] = (i >> 6) == w ? 1ull << (i & 63) : 0ull;
    for (int depth = 1; depth <= W * 64; ++depth) {
        unsigned long long nx[W];
#pragma unroll
        for (int w = 0; w < W; ++w) nx[w] = 0ull;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            unsigned long long f = fr[w];
            while (f) {
                const int u = w * 64 + __builtin_ctzll(f);
                f &= f - 1;
#pragma unroll
                for (int v = 0; v < W; ++v) {
                    unsigned long long a = adj[u * W + v];
                    if (u == i && v == jw) a &= ~jbit;                          // the bond itself is removed
                    nx[v] |= a;
                }
            }
        }
        bool hit = false, any = false;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            nx[w] &= ~vis[w];
            hit |= w == jw && (nx[w] & jbit);
            any |= nx[w] != 0ull;
            vis[w] |= nx[w];
            fr[w] = nx[w];
        }
        if (hit) return depth + 1;
        if (!any) return 0;
    }
    return 0;
}

// PASS 0: the bonds of every (frame, molecule) into a.count.  PASS 1: everything else, with a.offset from the scan
template <int TEAM, int PASS>
__global__ __launch_bounds__(kMolThreads) void mgraph_kernel(MgraphArgs a) {
    constexpr int JPB = kMolThreads / TEAM, CAP = TEAM, W = CAP / 64;
    __shared__ double s_x[JPB * CAP], s_y[JPB * CAP], s_z[JPB * CAP];
    __shared__ double s_thr[3 * kMolMaxElements * kMolMaxElements];
    __shared__ double s_cc[PASS ? kMolMaxEdges + 1 : 1], s_all[PASS ? kMolMaxEdges + 1 : 1], s_bl[PASS ? kMolMaxEdges + 1 : 1];
    __shared__ unsigned long long s_adj[PASS ? JPB * CAP * W : 1];
    __shared__ int s_label[PASS ? JPB * CAP : 1], s_start[PASS ? JPB * CAP : 1];
    __shared__ unsigned s_hcc[PASS ? kMolMaxEdges + 1 : 1], s_hall[PASS ? kMolMaxEdges + 1 : 1], s_cls[kMolMaxClasses];
    __shared__ unsigned s_fc[1 + kMgraphRingBits];
    __shared__ int s_w[4];
    __shared__ unsigned char s_e[JPB * CAP], s_slot[kMolMaxClasses];
    const int tid = threadIdx.x, team = tid / TEAM, lane = tid % TEAM;
    const int frame = blockIdx.x / a.b.gx, bx = blockIdx.x % a.b.gx;
    const int E = a.r.E, EE = E * E;
    mol_stage(a.r, PASS != 0, s_thr, s_slot, s_cls, s_cc, s_all, s_hcc, s_hall);
    if (PASS) {
        for (int i = tid; i < a.n_bl; i += kMolThreads) s_bl[i] = a.bl_edges[i];
        if (tid <= kMgraphRingBits) s_fc[tid] = 0;
    }
    double *x = s_x + team * CAP, *y = s_y + team * CAP, *z = s_z + team * CAP;
    unsigned char *el = s_e + team * CAP;
    unsigned long long *adj = s_adj + (PASS ? team * CAP * W : 0);
    int *label = s_label + (PASS ? team * CAP : 0), *start = s_start + (PASS ? team * CAP : 0);
    for (int it = 0; it < a.b.iters; ++it) {
        const MolJob job = mol_job<JPB>(a.b, it, bx, team, frame);
        const bool active = job.active;
        const int n = job.n, moff = job.off;
        const size_t base = job.base, fm = (size_t)frame * (size_t)a.b.B + (size_t)job.m;
        __syncthreads();                  // the tables are written; the iteration before has read its molecule
        const int i = lane;
        const bool mine = i < n;
        // the classes are counted below, for complete molecules only; a bad one is flagged once, by the fill pass
        const int cl = mine ? mol_load_atom(a.b, a.r, base + i, i, PASS != 0, s_slot, x, y, z, el) : -1;
        __syncthreads();
        // ---- row i of the adjacency, in registers
        unsigned long long row[W];
#pragma unroll
        for (int w = 0; w < W; ++w) row[w] = 0ull;
        double xi = 0, yi = 0, zi = 0;
        int ei = 0, sum = 0;
        if (mine) { xi = x[i]; yi = y[i]; zi = z[i]; ei = el[i]; }
        const double *t1 = s_thr + ei * E, *t2 = t1 + EE, *t3 = t2 + EE;
        if (mine) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const int hi = n - w * 64 < 64 ? n - w * 64 : 64;
                for (int jj = 0; jj < hi; ++jj) {
                    const int j = w * 64 + jj;
                    if (j == i) continue;
                    double d;
                    const int o = mol_pair(xi, yi, zi, x[j], y[j], z[j], t1, t2, t3, el[j], d);
                    sum += o;
                    if (o) row[w] |= 1ull << jj;
                }
            }
        }
        int up = 0, deg = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) { up += __popcll(mg_above<W>(row[w], w, i)); deg += __popcll(row[w]); }
        if (!PASS) {
            const int nb = mg_reduce<TEAM>(up, MgSum(), s_w);
            if (active && lane == 0) a.count[fm] = nb;
            continue;                     // uniform over the workgroup: PASS is a template argument
        }
        if (mine) {
#pragma unroll
            for (int w = 0; w < W; ++w) adj[i * W + w] = row[w];
            label[i] = i;
            a.nr_bonds[base + i] = sum;
            a.degree[base + i] = deg;
        }
        const int first = mg_scan<TEAM>(up, s_w);
        const int nb = mg_reduce<TEAM>(up, MgSum(), s_w);
        if (mine) start[i] = first;
        __syncthreads();                  // adjacency, labels and starts are in LDS
        // ---- fragments: every atom takes the smallest label among itself and its neighbours, then its label's label, in place,
        // until a sweep changes nothing.  Labels only fall and stay atoms of the fragment, so the fixed point is the smallest index
        for (int sweep = 0; sweep <= CAP; ++sweep) {
            int changed = 0;
            if (mine) {
                const int old = label[i];
                int l = old;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    unsigned long long r = row[w];
                    while (r) {
                        const int lj = label[w * 64 + __builtin_ctzll(r)];
                        r &= r - 1;
                        l = lj < l ? lj : l;
                    }
                }
                const int ll = label[l];
                l = ll < l ? ll : l;
                if (l < old) { label[i] = l; changed = 1; }
            }
            if (!__syncthreads_or(changed)) break;
        }
        int size = 0, lab = 0;
        if (mine) {
            lab = label[i];
            for (int j = 0; j < n; ++j) size += label[j] == lab;
            a.frag[base + i] = moff + lab;
        }
        const int n_frags = mg_reduce<TEAM>(mine && lab == i ? 1 : 0, MgSum(), s_w);
        const int largest = mg_reduce<TEAM>(size, MgMax(), s_w);
        const bool complete = active && n_frags == 1;
        // ---- bonds of atom i to higher atoms: the list entry, the bond-length bins, the ring through the bond
        const long long o0 = active ? a.offset[fm] : 0;
        int rmin = 0;
        unsigned rbits = 0;
        if (mine) {
            long long k = o0 + first;
            const int np = E * (E + 1) / 2, nbin = a.n_bl + 1;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                unsigned long long r = mg_above<W>(row[w], w, i);
                while (r) {
                    const int j = w * 64 + __builtin_ctzll(r);
                    r &= r - 1;
                    double d;
                    const int ej = el[j];
                    const int o = mol_pair(xi, yi, zi, x[j], y[j], z[j], t1, t2, t3, ej, d);
                    const int ring = mg_ring<W>(adj, i, j);
                    a.bonds[3 * k] = moff + i; a.bonds[3 * k + 1] = moff + j; a.bonds[3 * k + 2] = o;
                    a.ring_bond[k] = ring;
                    ++k;
                    if (ring) {
                        rmin = rmin && rmin < ring ? rmin : ring;
                        rbits |= 1u << (ring < kMgraphRingBits - 1 ? ring : kMgraphRingBits - 1);
                    }
                    if (o < 1) continue;  // cannot happen: the row bit came from the same statements
                    const int lo = ei < ej ? ei : ej, hi = ei < ej ? ej : ei;
                    const size_t cell = (((size_t)(lo * E - lo * (lo - 1) / 2 + (hi - lo))) * 3 + (o - 1)) * nbin + mol_bin(s_bl, a.n_bl, d);
                    unsigned long long *h = a.hist_bl + (size_t)frame * 2 * np * 3 * nbin;
                    atomicAdd(&h[cell], 1ull);
                    if (complete) atomicAdd(&h[(size_t)np * 3 * nbin + cell], 1ull);
                }
            }
        }
        const unsigned mol_bits = (unsigned)mg_reduce<TEAM>((int)rbits, MgOr(), s_w);
        __syncthreads();                  // this workgroup's ring_bond entries are written (and visible to it)
        if (mine) {
            // bonds to lower atoms j: entry offset + start[j] + (rank of i among j's higher neighbours)
#pragma unroll
            for (int w = 0; w < W; ++w) {
                unsigned long long r = row[w] & ~mg_above<W>(row[w], w, i);
                while (r) {
                    const int j = w * 64 + __builtin_ctzll(r);
                    r &= r - 1;
                    int rank = 0;
#pragma unroll
                    for (int v = 0; v < W; ++v) {
                        unsigned long long aj = mg_above<W>(adj[j * W + v], v, j);
                        const int iw = i >> 6;
                        if (v > iw) aj = 0ull;
                        if (v == iw) aj &= (1ull << (i & 63)) - 1ull;
                        rank += __popcll(aj);
                    }
                    const int ring = a.ring_bond[o0 + start[j] + rank];
                    if (ring) rmin = rmin && rmin < ring ? rmin : ring;
                }
            }
            a.ring_atom[base + i] = rmin;
            if (complete && cl >= 0) atomicAdd(&s_cls[cl], 1u);
        }
        // ---- pair-distance histograms of complete molecules
        if (mine && complete) {
            const bool ci = ei == a.r.carbon;
            for (int j = i + 1; j < n; ++j) {
                double d;
                const int ej = el[j];
                (void)mol_pair(xi, yi, zi, x[j], y[j], z[j], t1, t2, t3, ej, d);
                mol_hist_add(a.r, ci, ej, d, s_cc, s_all, s_hcc, s_hall);
            }
        }
        if (active && lane == 0) {
            int *mo = a.mol_out + 6 * fm;
            mo[0] = nb; mo[1] = n_frags; mo[2] = largest; mo[3] = complete; mo[4] = nb - n + n_frags; mo[5] = (int)mol_bits;
            if (complete) atomicAdd(&s_fc[0], 1u);
            for (int s = 0; s < kMgraphRingBits; ++s)
                if (mol_bits >> s & 1u) atomicAdd(&s_fc[1 + s], 1u);
        }
    }
    if (!PASS) return;
    __syncthreads();
    mol_flush(a.r, a.o, frame, s_hcc, s_hall, s_cls);
    if (tid <= kMgraphRingBits && s_fc[tid]) atomicAdd(&a.frame_counts[(size_t)frame * (1 + kMgraphRingBits) + tid], (unsigned long long)s_fc[tid]);
}

// One workgroup: exclusive scan of the n counts into offset (n + 1, 64-bit), kMgraphScanItems consecutive counts per thread and
// a carry from pass to pass; offset[n] is the total
__global__ __launch_bounds__(kMolThreads) void mgraph_scan_kernel(const int *count, long long *offset, long long n) {
    __shared__ long long s_wave[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long carry = 0;
    for (long long base = 0; base < n; base += (long long)kMolThreads * kMgraphScanItems) {
        const long long first = base + (long long)threadIdx.x * kMgraphScanItems;
        int c[kMgraphScanItems];
        long long v = 0;
#pragma unroll
        for (int q = 0; q < kMgraphScanItems; ++q) { c[q] = first + q < n ? count[first + q] : 0; v += c[q]; }
        long long inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        __syncthreads();                  // s_wave may still be read from the pass before
        if (lane == 63) s_wave[w] = inc;
        __syncthreads();
        long long ex = carry + inc - v, total = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < w) ex += s_wave[q];
            total += s_wave[q];
        }
#pragma unroll
        for (int q = 0; q < kMgraphScanItems; ++q) {
            if (first + q < n) offset[first + q] = ex;
            ex += c[q];
        }
        carry += total;
    }
    if (threadIdx.x == 0) offset[n] = carry;
}

#endif  // device code

// Checks a call and lays out its two launch forms.  "" or the refusal's message; `out` may be null.
inline std::string mgraph_plan(int64_t F, int64_t B, const int64_t *off, int E, int C, const int32_t *class_slot, const double *cc_edges, int n_cc,
                               double cc_cut, const double *all_edges, int n_all, double all_cut, const double *bl_edges, int n_bl, MolPlan *out) {
    return mol_plan("bond graph", kMgraphMaxAtoms, F, B, off, E, C, class_slot,
                    {{"C-C", cc_edges, n_cc, cc_cut}, {"all-pairs", all_edges, n_all, all_cut}, {"bond-length", bl_edges, n_bl, 0.0}}, out);
}
