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
// ---------------------------------------------------------------------------------------------
#pragma once
#include "sm_device.h"

enum CfgType { CFG_NONE = 0, CFG_REFERENCE = 1, CFG_DYNAMIC = 2, CFG_RESCALE = 3 };

constexpr int kCfgBins = 2048;            // radix digits of 11 bits
constexpr int kCfgMaxBlocks = 256;        // workgroups of the partial-sum and histogram kernels (per tensor)
constexpr int kCfgHistWords = 3 * kCfgBins + 8;     // per tensor: three histograms, min-above, pass states
constexpr int kCfgShift[3] = {21, 10, 0};

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
    float *stat;                  // [2] s or r of the positions | of the logits
    double *part;                 // [2][kCfgMaxBlocks][4] partial sums
    unsigned *hist;               // [2][kCfgHistWords]
    int blocks[2];                // workgroups per tensor
    long long k_lo[2], k_hi[2];   // quantile: neighbouring ranks (torch.quantile's float32 rank q * (n - 1))
    float weight[2];              // ... and the interpolation weight rank - k_lo
};

SM_DEV unsigned cfg_key(float x) {        // order-preserving: key(a) < key(b) <=> a < b (NaN-free)
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SM_DEV float cfg_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// element e of tensor `which` (0 positions, 1 logits): the combined value and the conditional one
SM_DEV float cfg_combine(const CfgArgs &a, float c, float u) {
#pragma clang fp contract(off)
    return a.w1 * c - a.w * u;
}
SM_DEV void cfg_load(const CfgArgs &a, int which, long long e, float &x, float &c) {
    const float *pc = which ? a.v_c : a.pos_c, *pu = which ? a.v_u : a.pos_u;
    c = pc[e];
    x = cfg_combine(a, c, pu[e]);
}
SM_DEV long long cfg_count(const CfgArgs &a, int which) { return (long long)a.n_atoms * (which ? a.C : 3); }

// threshold_CFG of one value: `stat` is s or r of its tensor; k >= 0 (the coordinate) clamps into the box
SM_DEV float cfg_apply(const CfgArgs &a, float x, float stat, int k) {
#pragma clang fp contract(off)
    if (a.type == CFG_REFERENCE || a.type == CFG_DYNAMIC) x = fminf(fmaxf(x, -stat), stat);
    else if (a.type == CFG_RESCALE) x = a.pf * (x * stat) + a.qf * x;
    if (k >= 0 && a.has_bounds) {      // (selects, not an indexed load: a dynamic index would put the argument block in scratch)
        const float lo = k == 0 ? a.lo[0] : (k == 1 ? a.lo[1] : a.lo[2]), hi = k == 0 ? a.hi[0] : (k == 1 ? a.hi[1] : a.hi[2]);
        x = fminf(fmaxf(x, lo), hi);
    }
    return x;
}

// reference_threshold / rescale: per-workgroup float64 partials.  grid (blocks, 2), 256 threads.
// part[which][block] = {max|c|, 0, 0, 0} or {sum x, sum x^2, sum c, sum c^2}
__global__ void __launch_bounds__(256) cfg_partial_kernel(CfgArgs a) {
    const int which = blockIdx.y;
    if ((int)blockIdx.x >= a.blocks[which]) return;
    const long long n = cfg_count(a, which);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)a.blocks[which] * 256) {
        float x, c;
        cfg_load(a, which, e, x, c);
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
    if (threadIdx.x < 4) a.part[((size_t)which * kCfgMaxBlocks + blockIdx.x) * 4 + threadIdx.x] = red[threadIdx.x][0];
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
// hist[which]: [0..3*kCfgBins) histograms, [3*kCfgBins] ~min key above the final prefix, [+1..+4] (prefix, rank) after
// passes 0 and 1 (low / high 32 bits of the rank: ranks < 2^31 here)
template <int PASS>
__global__ void __launch_bounds__(256) cfg_hist_kernel(CfgArgs a) {
    const int which = blockIdx.y;
    if ((int)blockIdx.x >= a.blocks[which]) return;
    unsigned *H = a.hist + (size_t)which * kCfgHistWords;
    __shared__ unsigned lh[kCfgBins];
    for (int j = threadIdx.x; j < kCfgBins; j += 256) lh[j] = 0u;
    unsigned prefix = 0;
    if (PASS > 0) {      // the digit of the previous pass, from its merged histogram (pass 1: 11-bit prefix, pass 2: 22-bit)
        const unsigned prev_prefix = PASS == 1 ? 0u : H[3 * kCfgBins + 1];
        const long long krem = PASS == 1 ? a.k_lo[which] : (long long)H[3 * kCfgBins + 2];
        const CfgDigit dg = cfg_find_digit(H + (PASS - 1) * kCfgBins, krem);
        prefix = (prev_prefix << 11) | (unsigned)(dg.d < 0 ? 0 : dg.d);
        if (blockIdx.x == 0 && threadIdx.x == 0) {      // the state the next pass / the finalize kernel starts from
            H[3 * kCfgBins + 1 + 2 * (PASS - 1)] = prefix;
            H[3 * kCfgBins + 2 + 2 * (PASS - 1)] = (unsigned)dg.krem;
        }
    }
    __syncthreads();
    const long long n = cfg_count(a, which);
    const int sh = kCfgShift[PASS], psh = PASS > 0 ? kCfgShift[PASS - 1] : 32;
    const unsigned mask = PASS == 2 ? 1023u : 2047u;
    unsigned above = 0u;      // max of ~key over the keys above the final prefix (PASS 2)
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)a.blocks[which] * 256) {
        float x, c;
        cfg_load(a, which, e, x, c);
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

// the statistic of each tensor from the partials or the histograms; clears the histograms.  grid 2, 256 threads.
__global__ void __launch_bounds__(256) cfg_finalize_kernel(CfgArgs a) {
    const int which = blockIdx.x, t = threadIdx.x;
    const long long n = cfg_count(a, which);
    if (a.type == CFG_DYNAMIC) {
        unsigned *H = a.hist + (size_t)which * kCfgHistWords;
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
            if (a.k_hi[which] != a.k_lo[which] && dg.krem + 1 >= (long long)dg.cnt)      // the next rank holds a larger key
                key_hi = next_bin < 1024 ? (prefix << 10) | (unsigned)next_bin : ~H[3 * kCfgBins];
            const float lo = cfg_unkey(key_lo), hi = cfg_unkey(key_hi), wgt = a.weight[which];
            // torch.lerp (ATen/native/Lerp.h): two branches on |weight| < 0.5, each one fused multiply-add
            const float s = fabsf(wgt) < 0.5f ? fmaf(wgt, hi - lo, lo) : fmaf(-(hi - lo), 1.0f - wgt, hi);
            a.stat[which] = s;
        }
        __syncthreads();
        for (int j = t; j < kCfgHistWords; j += 256) H[j] = 0u;     // ready for the next step
        return;
    }
    __shared__ double red[4][256];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = t; b < a.blocks[which]; b += 256)
        for (int j = 0; j < 4; ++j) {
            const double v = a.part[((size_t)which * kCfgMaxBlocks + b) * 4 + j];
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
            a.stat[which] = (float)red[0][0] * a.pf;
        } else {       // torch.std: unbiased; each standard deviation rounded to float32, then the float32 ratio
            const double nd = (double)n;
            const double vx = (red[1][0] - red[0][0] * red[0][0] / nd) / (nd - 1.0);
            const double vc = (red[3][0] - red[2][0] * red[2][0] / nd) / (nd - 1.0);
            const float sx = (float)sqrt(vx > 0.0 ? vx : 0.0), sc = (float)sqrt(vc > 0.0 ? vc : 0.0);
            a.stat[which] = n > 1 ? sc / sx : __int_as_float(0x7fc00000);
        }
    }
}
