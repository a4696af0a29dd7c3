// Classifier-free guidance (models/molopt_score_model.py:616-642, threshold_CFG :116-151).  Per reverse step the chain runs
// the score twice, with the shape condition and with a zeroed one, and combines the two predictions
//     x = (1 + w) * cond - w * uncond
// for the positions (N*3 values) and the atom-type logits (N*C values).  threshold_CFG then rescales or clips x with ONE
// statistic of the whole flattened batch tensor, and clamps the positions into the box of molecule 0:
//   reference_threshold  s = max|cond| * p                      clip(x, -s, s)
//   dynamic_threshold    s = torch.quantile(x, p)               clip(x, -s, s)
//   rescale              r = std(cond) / std(x) (unbiased)      p * (x * r) + (1 - p) * x
// The statistic stage below writes s (or r) of both tensors to a two-float device buffer; the posterior-step kernel
// (ddpm_step16_kernel / ddpm_step_kernel, sm_misc.h) recomputes x from the two predictions, applies the threshold and the
// clamp, and consumes the result.  Every operation is rounded as torch rounds it in float32 (no FMA contraction): the scalars
// (1 + w), w, p and (1 - p) are formed in double and rounded to float32 once, as torch's wrapped Python scalars are.
//
// Statistic stage:
//   max|cond|, the sums of the standard deviations: per-workgroup float64 partials (cfg_partial_kernel), reduced in a fixed
//   order by one workgroup per tensor (cfg_finalize_kernel): deterministic, no floating-point atomics.
//   quantile: exact order-statistic selection, a radix select on order-preserving uint32 keys in three passes of 11, 11 and
//   10 bits (cfg_hist_kernel).  Each pass builds per-workgroup LDS histograms of the keys that share the prefix chosen so far
//   and merges them into a global histogram with integer atomics; every workgroup of the next pass re-derives the chosen digit
//   from that histogram (all arrive at the same answer), so no extra launch picks it.  The last pass also keeps the smallest
//   key above the final 22-bit prefix (an atomic max of ~key), which gives the next order statistic when the rank's
//   neighbour lies outside the last histogram.  cfg_finalize_kernel resolves both neighbouring ranks and interpolates with
//   torch.lerp's formula; it then clears the histograms for the next step.
//
// Groups (shapemol_set_cfg_groups): the chain's molecules are cut into contiguous groups, each with its own strength w_g and its
// own box, and every statistic above is taken over ONE group's elements.  A group is a contiguous run of atoms (the batch vector
// is sorted), so of elements of both tensors.  Per group, in device memory (CfgGroup): the scalars the host rounds once, and
// what cfg_groups_table_kernel derives once per chain from the batch vector -- per tensor the element range, the first
// workgroup and the workgroup count, the quantile's ranks and weight (float32 rank, __fmul_rn: no contraction) -- together with
// a molecule -> group table and a workgroup -> (group, local workgroup) table per tensor.
//   Independence rule: group g gets the workgroup count the one-group chain of its elements would get, max(1, ceil(n / 2048))
//   capped at kCfgMaxBlocks, the same strided element order inside them, its own partials, its own histogram set
//   (kCfgHistWords per (group, tensor)) and the same fixed-order final reduction: a group's statistic is a function of its own
//   elements and their count alone, bit for bit the statistic of the one-group chain of that slice (float64 sums included).
//   Launch grids come from a host-side bound, sum over the groups of the workgroups <= n / 2048 + G per tensor; the tables'
//   tail is marked idle (group -1).  The finalize kernel runs on a (tensor, group) grid and writes stat[g][2].
//   A group with w_g = 0 has type CFG_NONE and no box in its row: it consumes its raw conditional prediction (the reference's
//   `else` branch); it gets no workgroups, and the finalize kernel writes the identity (s = +inf, r = 1) for it.
//   At most kCfgMaxGroups groups per chain (the histograms are 2 * kCfgHistWords * 4 B = 49 KB per group).
// The same kernels serve both forms: CfgArgs::grp == nullptr is the whole-batch form, one segment per tensor.
// ---------------------------------------------------------------------------------------------
#pragma once
#include "sm_device.h"

enum CfgType { CFG_NONE = 0, CFG_REFERENCE = 1, CFG_DYNAMIC = 2, CFG_RESCALE = 3 };

constexpr int kCfgBins = 2048;            // radix digits of 11 bits
constexpr int kCfgMaxBlocks = 256;        // workgroups of the partial-sum and histogram kernels (per tensor and group)
constexpr int kCfgHistWords = 3 * kCfgBins + 8;     // per tensor and group: three histograms, min-above, pass states
constexpr int kCfgShift[3] = {21, 10, 0};
constexpr int kCfgMaxGroups = 256;        // groups of a chain (shapemol_set_cfg_groups refuses more): 12.6 MB of histograms

// one group of a chain (device memory; G + 1 rows, row G holds only mol0 = the number of molecules)
struct alignas(16) CfgGroup {
    // from the host (shapemol_set_cfg_groups): three 16-byte words, which the posterior step reads with one load each
    float w1, w;                  // (float)(1 + w_g), (float)w_g
    int type;                     // the chain's CfgType, or CFG_NONE for w_g = 0 (raw conditional prediction)
    int has_box;                  // 0 for w_g = 0 or a NaN box
    float lo[3]; int mol0;        // the group's box: lower corner | first molecule
    float hi[3]; int pad;         // ... upper corner
    // from cfg_groups_table_kernel, per tensor (0 positions, 1 logits)
    long long e0[2], n[2];        // element range [e0, e0 + n)
    long long k_lo[2], k_hi[2];   // quantile: neighbouring ranks inside the group
    int blk0[2], nblk[2];         // first workgroup, workgroups (0: no statistic -- w_g = 0, or no element)
    float weight[2];              // the quantile's interpolation weight
};

static_assert(offsetof(CfgGroup, lo) == 16 && offsetof(CfgGroup, hi) == 32 && sizeof(CfgGroup) % 16 == 0, "CfgGroup: the host part is three 16-byte words");

struct CfgArgs {
    const float *pos_c, *pos_u;   // [N][3] conditional / unconditional predicted positions
    const float *v_c, *v_u;       // [N][C] conditional / unconditional predicted logits
    float w1, w;                  // (float)(1 + w), (float)w
    float pf, qf;                 // (float)p, (float)(1 - p)
    float lo[3], hi[3];           // box of molecule 0 (bounds[0][:, 0], bounds[0][:, 1])
    int has_bounds;
    int type;                     // CfgType
    int on;                       // 0: the posterior step is the unguided one
    int n_atoms, C;
    float *stat;                  // [2] s or r of the positions | of the logits; groups: [G][2]
    double *part;                 // [2][kCfgMaxBlocks][4] partial sums; groups: [2][tab_stride][4]
    unsigned *hist;               // [2][kCfgHistWords]; groups: [G][2][kCfgHistWords]
    int blocks[2];                // workgroups per tensor; groups: the host-side bound the grid is sized by
    long long k_lo[2], k_hi[2];   // quantile: neighbouring ranks (torch.quantile's float32 rank q * (n - 1))
    float weight[2];              // ... and the interpolation weight rank - k_lo
    // groups (nullptr / 0: the whole-batch form above; with groups w1, w, the box, k_lo, k_hi and weight above are unused)
    const CfgGroup *grp;          // [G + 1]
    const int *mol_grp;           // [B] molecule -> group
    const int2 *blk_tab;          // [2][tab_stride] workgroup -> (group or -1, local workgroup)
    int n_groups, tab_stride;
};

SM_DEV unsigned cfg_key(float x) {        // order-preserving: key(a) < key(b) <=> a < b (NaN-free)
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SM_DEV float cfg_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

SM_DEV float cfg_combine(float w1, float w, float c, float u) {
#pragma clang fp contract(off)
    return w1 * c - w * u;
}

// What one lane of the posterior step needs of the guidance of its atom: the whole batch's values from the argument block, or
// those of the atom's group from its row (k = the lane's coordinate, 0..2: which side of the box it reads)
struct CfgLane { float w1, w, lo, hi, stat_pos, stat_v; int type, has_box; };
SM_DEV CfgLane cfg_lane(const CfgArgs &a, int mol, int k) {
    CfgLane L;
    if (a.grp) {       // (global memory: a dynamic index is an address, not a scratch copy of the argument block)
        const int g = a.mol_grp[mol];
        const float4 *row = reinterpret_cast<const float4 *>(a.grp + g);
        const float4 sc = row[0], lo = row[1], hi = row[2];
        const float2 st = *reinterpret_cast<const float2 *>(a.stat + 2 * g);
        L.w1 = sc.x; L.w = sc.y; L.type = __float_as_int(sc.z); L.has_box = __float_as_int(sc.w);
        L.lo = k == 0 ? lo.x : (k == 1 ? lo.y : lo.z); L.hi = k == 0 ? hi.x : (k == 1 ? hi.y : hi.z);
        L.stat_pos = st.x; L.stat_v = st.y;
    } else {       // (selects, not an indexed load: a dynamic index would put the argument block in scratch)
        L.w1 = a.w1; L.w = a.w; L.type = a.type; L.has_box = a.has_bounds;
        L.lo = k == 0 ? a.lo[0] : (k == 1 ? a.lo[1] : a.lo[2]); L.hi = k == 0 ? a.hi[0] : (k == 1 ? a.hi[1] : a.hi[2]);
        L.stat_pos = a.stat[0]; L.stat_v = a.stat[1];
    }
    return L;
}

// threshold_CFG of one value: `stat` is s or r of its tensor (and group); clamp: a coordinate, clamped into the box
SM_DEV float cfg_apply(const CfgArgs &a, const CfgLane &L, float x, float stat, bool clamp) {
#pragma clang fp contract(off)
    if (L.type == CFG_REFERENCE || L.type == CFG_DYNAMIC) x = fminf(fmaxf(x, -stat), stat);
    else if (L.type == CFG_RESCALE) x = a.pf * (x * stat) + a.qf * x;
    if (clamp && L.has_box) x = fminf(fmaxf(x, L.lo), L.hi);
    return x;
}

// One segment of the statistic stage: the elements of tensor `which` (0 positions, 1 logits) of the whole batch, or of one group
struct CfgSeg {
    long long e0, n;              // elements [e0, e0 + n) of the tensor
    int local, nblk;              // this workgroup among the segment's
    float w1, w;
    long long k_lo, k_hi; float weight;
    unsigned *H;                  // [kCfgHistWords]
    double *part;                 // [nblk][4]
    float *stat;
    int type;                     // CFG_NONE: no statistic (identity)
};
SM_DEV long long cfg_count(const CfgArgs &a, int which) { return (long long)a.n_atoms * (which ? a.C : 3); }
// the segment of group g (whole-batch form: g = 0), workgroup `local` of it
SM_DEV CfgSeg cfg_seg(const CfgArgs &a, int which, int g, int local) {
    CfgSeg s;
    s.local = local;
    if (a.grp) {
        const CfgGroup &G = a.grp[g];
        s.e0 = G.e0[which]; s.n = G.n[which]; s.nblk = G.nblk[which]; s.w1 = G.w1; s.w = G.w;
        s.k_lo = G.k_lo[which]; s.k_hi = G.k_hi[which]; s.weight = G.weight[which];
        s.H = a.hist + ((size_t)g * 2 + which) * kCfgHistWords;
        s.part = a.part + ((size_t)which * a.tab_stride + G.blk0[which]) * 4;
        s.stat = a.stat + 2 * g + which;
        s.type = s.nblk > 0 ? G.type : CFG_NONE;
    } else {
        s.e0 = 0; s.n = cfg_count(a, which); s.nblk = a.blocks[which]; s.w1 = a.w1; s.w = a.w;
        s.k_lo = a.k_lo[which]; s.k_hi = a.k_hi[which]; s.weight = a.weight[which];
        s.H = a.hist + (size_t)which * kCfgHistWords;
        s.part = a.part + (size_t)which * kCfgMaxBlocks * 4;
        s.stat = a.stat + which;
        s.type = a.type;
    }
    return s;
}
// the segment workgroup (blockIdx.x, tensor blockIdx.y) of a partial / histogram launch works on; false: an idle workgroup
SM_DEV bool cfg_block_seg(const CfgArgs &a, int which, CfgSeg &s) {
    if ((int)blockIdx.x >= a.blocks[which]) return false;
    if (!a.grp) { s = cfg_seg(a, which, 0, (int)blockIdx.x); return true; }
    const int2 e = a.blk_tab[(size_t)which * a.tab_stride + blockIdx.x];
    if (e.x < 0) return false;
    s = cfg_seg(a, which, e.x, e.y);
    return true;
}
// element e of the segment: the combined value and the conditional one
SM_DEV void cfg_load(const CfgArgs &a, int which, const CfgSeg &s, long long e, float &x, float &c) {
    const float *pc = which ? a.v_c : a.pos_c, *pu = which ? a.v_u : a.pos_u;
    c = pc[s.e0 + e];
    x = cfg_combine(s.w1, s.w, c, pu[s.e0 + e]);
}

// Once per chain, outside the captured step: the device half of the groups' rows, the molecule -> group table and the
// workgroup tables.  One workgroup of 256 threads.  grp[G + 1]: mol0 host-validated (starts at 0, does not decrease, row G =
// n_mols).  n_blk[2]: the launch bounds the workgroup tables are sized by (entries beyond the groups' workgroups: idle).
__global__ void __launch_bounds__(256) cfg_groups_table_kernel(const int64_t *batch, int n_atoms, int C, int n_groups, int n_mols, float pf,
                                                               CfgGroup *grp, int *mol_grp, int2 *blk_tab, int tab_stride, int n_blk0, int n_blk1) {
    __shared__ int aoff[kCfgMaxGroups + 1], mol0[kCfgMaxGroups + 1];
    if (n_groups > kCfgMaxGroups) return;
    for (int g = threadIdx.x; g <= n_groups; g += blockDim.x) {      // first atom whose molecule is >= mol0[g]
        const int64_t m = grp[g].mol0;
        mol0[g] = (int)m;
        int lo = 0, hi = n_atoms;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (batch[mid] < m) lo = mid + 1; else hi = mid;
        }
        aoff[g] = lo;
    }
    __syncthreads();
    if (threadIdx.x < 2) {        // one thread per tensor: the groups' workgroups back to back, in group order
        const int which = threadIdx.x, per = which ? C : 3, n_blk = which ? n_blk1 : n_blk0;
        int b = 0;
        for (int g = 0; g < n_groups; ++g) {
            const long long na = aoff[g + 1] - aoff[g];      // (negative only for an unsorted batch vector: no element then)
            const long long n = na > 0 ? na * per : 0;
            // the workgroup count of the one-group chain of these elements (shapemol_hip.hip, cfg_args)
            long long nb = (n + 2047) / 2048;
            nb = nb < 1 ? 1 : (nb > kCfgMaxBlocks ? kCfgMaxBlocks : nb);
            if (n == 0 || grp[g].type == CFG_NONE) nb = 0;
            if (b + nb > n_blk) nb = n_blk - b;              // (never by construction; keeps every write inside the tables)
            // torch.quantile: q rounded to float32, rank = q * (n - 1) in float32, the two ranks around it, weight rank - below
            const float last = (float)(n - 1);
            const float rank = n > 0 ? __fmul_rn(pf, last) : 0.f;
            long long k_lo = (long long)rank, k_hi = (long long)ceilf(rank);
            const float weight = __fsub_rn(rank, (float)k_lo);
            const long long top = n > 0 ? n - 1 : 0;
            k_lo = k_lo < 0 ? 0 : (k_lo > top ? top : k_lo);
            k_hi = k_hi < 0 ? 0 : (k_hi > top ? top : k_hi);
            CfgGroup &G = grp[g];
            G.e0[which] = (long long)aoff[g] * per; G.n[which] = n; G.blk0[which] = b; G.nblk[which] = (int)nb;
            G.k_lo[which] = k_lo; G.k_hi[which] = k_hi; G.weight[which] = weight;
            for (int j = 0; j < (int)nb; ++j) blk_tab[(size_t)which * tab_stride + b + j] = make_int2(g, j);
            b += (int)nb;
        }
        for (; b < n_blk; ++b) blk_tab[(size_t)which * tab_stride + b] = make_int2(-1, 0);
    }
    for (int m = threadIdx.x; m < n_mols; m += blockDim.x) {       // the last group whose first molecule is <= m
        int lo = 0, hi = n_groups - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (mol0[mid] <= m) lo = mid; else hi = mid - 1;
        }
        mol_grp[m] = lo;
    }
}

// reference_threshold / rescale: per-workgroup float64 partials.  grid (blocks, 2), 256 threads.
// part[which][block] = {max|c|, 0, 0, 0} or {sum x, sum x^2, sum c, sum c^2}
__global__ void __launch_bounds__(256) cfg_partial_kernel(CfgArgs a) {
    const int which = blockIdx.y;
    CfgSeg sg;
    if (!cfg_block_seg(a, which, sg)) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long e = (long long)sg.local * 256 + threadIdx.x; e < sg.n; e += (long long)sg.nblk * 256) {
        float x, c;
        cfg_load(a, which, sg, e, x, c);
        if (a.type == CFG_REFERENCE) {
            s[0] = fmax(s[0], (double)fabsf(c));
        } else {
            const double xd = x, cd = c;
            s[0] += xd; s[1] += xd * xd; s[2] += cd; s[3] += cd * cd;
        }
    }
    __shared__ double red[4][256];
    for (int j = 0; j < 4; ++j) red[j][threadIdx.x] = s[j];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int j = 0; j < 4; ++j)
                red[j][threadIdx.x] = a.type == CFG_REFERENCE ? fmax(red[j][threadIdx.x], red[j][threadIdx.x + h])
                                                              : red[j][threadIdx.x] + red[j][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < 4) sg.part[(size_t)sg.local * 4 + threadIdx.x] = red[threadIdx.x][0];
}

// the digit of a pass that holds rank `krem` among the keys of histogram h (256 threads, 8 bins each), the rank left
// inside that digit and the digit's count; every thread of the workgroup gets the same answer
struct CfgDigit { int d; long long krem; unsigned cnt; };
SM_DEV CfgDigit cfg_find_digit(const unsigned *h, long long krem) {
    __shared__ long long scan[256];
    __shared__ CfgDigit res;
    const int t = threadIdx.x;
    unsigned loc = 0;
    for (int j = 0; j < 8; ++j) loc += h[t * 8 + j];
    scan[t] = loc;
    if (t == 0) res = CfgDigit{-1, 0, 0u};
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {      // inclusive scan
        const long long v = t >= off ? scan[t - off] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    long long before = t ? scan[t - 1] : 0;
    if (krem >= before && krem < scan[t]) {
        for (int j = 0; j < 8; ++j) {
            const unsigned c = h[t * 8 + j];
            if (krem < before + c) { res = CfgDigit{t * 8 + j, krem - before, c}; break; }
            before += c;
        }
    }
    __syncthreads();
    const CfgDigit r = res;
    __syncthreads();
    return r;
}

// one radix pass (PASS 0, 1, 2) of the quantile's lower rank.  grid (blocks, 2), 256 threads.
// H (per tensor and group): [0..3*kCfgBins) histograms, [3*kCfgBins] ~min key above the final prefix, [+1..+4] (prefix, rank)
// after passes 0 and 1 (low / high 32 bits of the rank: ranks < 2^31 here)
template <int PASS>
__global__ void __launch_bounds__(256) cfg_hist_kernel(CfgArgs a) {
    const int which = blockIdx.y;
    CfgSeg sg;
    if (!cfg_block_seg(a, which, sg)) return;
    unsigned *H = sg.H;
    __shared__ unsigned lh[kCfgBins];
    for (int j = threadIdx.x; j < kCfgBins; j += 256) lh[j] = 0u;
    unsigned prefix = 0;
    if (PASS > 0) {      // the digit of the previous pass, from its merged histogram (pass 1: 11-bit prefix, pass 2: 22-bit)
        const unsigned prev_prefix = PASS == 1 ? 0u : H[3 * kCfgBins + 1];
        const long long krem = PASS == 1 ? sg.k_lo : (long long)H[3 * kCfgBins + 2];
        const CfgDigit dg = cfg_find_digit(H + (PASS - 1) * kCfgBins, krem);
        prefix = (prev_prefix << 11) | (unsigned)(dg.d < 0 ? 0 : dg.d);
        if (sg.local == 0 && threadIdx.x == 0) {      // the state the next pass / the finalize kernel starts from
            H[3 * kCfgBins + 1 + 2 * (PASS - 1)] = prefix;
            H[3 * kCfgBins + 2 + 2 * (PASS - 1)] = (unsigned)dg.krem;
        }
    }
    __syncthreads();
    const int sh = kCfgShift[PASS], psh = PASS > 0 ? kCfgShift[PASS - 1] : 32;
    const unsigned mask = PASS == 2 ? 1023u : 2047u;
    unsigned above = 0u;      // max of ~key over the keys above the final prefix (PASS 2)
    for (long long e = (long long)sg.local * 256 + threadIdx.x; e < sg.n; e += (long long)sg.nblk * 256) {
        float x, c;
        cfg_load(a, which, sg, e, x, c);
        const unsigned key = cfg_key(x);
        const unsigned top = PASS > 0 ? key >> psh : 0u;
        if (top == prefix) atomicAdd(&lh[(key >> sh) & mask], 1u);
        else if (PASS == 2 && top > prefix) above = max(above, ~key);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < kCfgBins; j += 256)
        if (lh[j]) atomicAdd(&H[PASS * kCfgBins + j], lh[j]);
    if (PASS == 2) {
        for (int off = 32; off > 0; off >>= 1) above = max(above, (unsigned)__shfl_xor((int)above, off));
        if ((threadIdx.x & 63) == 0 && above) atomicMax(&H[3 * kCfgBins], above);
    }
}

// the statistic of each tensor (and group) from the partials or the histograms; clears the histograms.
// grid 2 (whole batch) or (2, G), 256 threads.
__global__ void __launch_bounds__(256) cfg_finalize_kernel(CfgArgs a) {
    const int which = blockIdx.x, t = threadIdx.x;
    const CfgSeg sg = cfg_seg(a, which, (int)blockIdx.y, 0);
    if (sg.type == CFG_NONE) {      // a group without a statistic (w_g = 0, or no element): the identity
        if (t == 0) *sg.stat = a.type == CFG_RESCALE ? 1.0f : INFINITY;
        return;
    }
    const long long n = sg.n;
    if (a.type == CFG_DYNAMIC) {
        unsigned *H = sg.H;
        const unsigned prefix = H[3 * kCfgBins + 3];
        const long long krem = (long long)H[3 * kCfgBins + 4];
        const CfgDigit dg = cfg_find_digit(H + 2 * kCfgBins, krem);
        __shared__ int next_bin;      // the first non-empty bin above the digit (the next larger key inside the prefix)
        if (t == 0) next_bin = 1 << 30;
        __syncthreads();
        for (int j = t; j < 1024; j += 256)
            if (j > dg.d && H[2 * kCfgBins + j]) atomicMin(&next_bin, j);
        __syncthreads();
        if (t == 0) {
            const unsigned key_lo = (prefix << 10) | (unsigned)dg.d;
            unsigned key_hi = key_lo;
            if (sg.k_hi != sg.k_lo && dg.krem + 1 >= (long long)dg.cnt)      // the next rank holds a larger key
                key_hi = next_bin < 1024 ? (prefix << 10) | (unsigned)next_bin : ~H[3 * kCfgBins];
            const float lo = cfg_unkey(key_lo), hi = cfg_unkey(key_hi), wgt = sg.weight;
            // torch.lerp (ATen/native/Lerp.h): two branches on |weight| < 0.5, each one fused multiply-add
            const float s = fabsf(wgt) < 0.5f ? fmaf(wgt, hi - lo, lo) : fmaf(-(hi - lo), 1.0f - wgt, hi);
            *sg.stat = s;
        }
        __syncthreads();
        for (int j = t; j < kCfgHistWords; j += 256) H[j] = 0u;     // ready for the next step
        return;
    }
    __shared__ double red[4][256];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = t; b < sg.nblk; b += 256)
        for (int j = 0; j < 4; ++j) {
            const double v = sg.part[(size_t)b * 4 + j];
            s[j] = a.type == CFG_REFERENCE ? fmax(s[j], v) : s[j] + v;
        }
    for (int j = 0; j < 4; ++j) red[j][t] = s[j];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h)
            for (int j = 0; j < 4; ++j)
                red[j][t] = a.type == CFG_REFERENCE ? fmax(red[j][t], red[j][t + h]) : red[j][t] + red[j][t + h];
        __syncthreads();
    }
    if (t == 0) {
#pragma clang fp contract(off)
        if (a.type == CFG_REFERENCE) {
            *sg.stat = (float)red[0][0] * a.pf;
        } else {       // torch.std: unbiased; each standard deviation rounded to float32, then the float32 ratio
            const double nd = (double)n;
            const double vx = (red[1][0] - red[0][0] * red[0][0] / nd) / (nd - 1.0);
            const double vc = (red[3][0] - red[2][0] * red[2][0] / nd) / (nd - 1.0);
            const float sx = (float)sqrt(vx > 0.0 ? vx : 0.0), sc = (float)sqrt(vc > 0.0 ? vc : 0.0);
            *sg.stat = n > 1 ? sc / sx : __int_as_float(0x7fc00000);
        }
    }
}
