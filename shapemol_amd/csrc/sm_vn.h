// The equivariant coordinate update of a layer (BaseH2XAttLayer, uni_transformer.py:153-162), written once for every kernel
// family of the sampler:
//     VN-linear     p = W_f z, d = W_d z per (atom, channel), z = [x_i | o_i (16 attention rows) | shape_b]  (shape_vn_layers.py:95-110)
//     statistics    batch sums of ||p|| + 1e-6 and its square per channel, in double, spread over kVnReplicas accumulators
//     apply         train-mode batch-norm of ||p|| (shape_vn_layers.py:41-61), VN-leaky-ReLU against d, mean over the channels,
//                   x += mean over the attention rows + mean over the channels
// Only straight-line per-element code lives here; the loops, the LDS addresses, the barriers and the launch geometry stay in
// the kernels that call it (DESIGN.md section 2 lists which kernel calls which function).  Every summation order is fixed
// here: the forms are compared bit for bit against each other by the tests.
#pragma once
#include "sm_device.h"

constexpr int kVnReplicas = 16;       // copies of the double accumulator [kVnReplicas][2][heads]: same-address atomics serialise
                                      // at the memory side; workgroup b adds to copy b % kVnReplicas
// doubles of reduction scratch behind the LDS images of the h2x kernels (host and device use the same formula)
__host__ __device__ constexpr int vn_red_doubles(int nwave, int hd) {
    return nwave * 64 > (2 + 2 * kVnReplicas) * hd ? nwave * 64 : (2 + 2 * kVnReplicas) * hd;
}

// h2x: the VN-linear + batch statistics fused behind the attention (EdgeFusedArgs::VnFuse, Edge16Args::vn, EdgeStreamArgs::vn)
struct VnFuse {
    const float *ps;            // [B][2][heads][3]
    const float *wf_x, *wd_x;   // [heads]
    const float *wf_o, *wd_o;   // [heads][16]
    const float *bn_g, *bn_b;   // [heads]
    const int *mol_of;
    float *pd;                  // [N][heads][6]
    double *acc;                // [kVnReplicas][2][heads], zeroed at the start of the evaluation
    unsigned *arrive;           // grid-barrier counter of this launch, zeroed likewise
    int *err;                   // set to 1 if the grid barrier timed out (workgroups not co-resident)
    float *x_out;               // [N][3]
    int enable;                 // 0 off, 1 whole update (grid barrier inside), 2 VN-linear + statistics only
};

// x2h: the apply step of the PREVIOUS layer folded into the kernel's prologue: the workgroup recomputes the new coordinates of
// every atom of the molecules its jobs touch (their neighbours live there) into an LDS table, from the p / d vectors and the
// batch sums the h2x kernel left behind, and writes those of its own atoms to global memory for the kernels that follow.
// Saves the vn_apply launch (5 us) of every layer but the last.
constexpr int kVnFoldCap = 256;       // atoms of the LDS coordinate table (the host enables the fold only if every span fits)
struct VnFold {
    const float *pd;          // [N][heads][6]
    const double *acc;        // [kVnReplicas][2][heads] batch sums of the previous layer
    const float *bn_g, *bn_b; // [heads]
    const float *xsum;        // [N][3] sum over the attention rows, written by the h2x epilogue
    const float *x_old;       // [N][3]
    float *x_new;             // [N][3]
    const int2 *mol_span;     // [N] first / one-past-last atom of each atom's molecule
    int *span_flag;           // status flag raised if a workgroup's molecule span exceeds the table
    int enable;
};

// ---- VN-linear -----------------------------------------------------------------------------------------------------
SM_DEV float vn_norm(const float *p) { return sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) + 1e-6f; }
SM_DEV void vn_norm_sums(const float *p, double &s1, double &s2) {
    const float nrm = vn_norm(p);
    s1 += (double)nrm;
    s2 += (double)nrm * (double)nrm;
}
// sum of coordinate c over the 16 attention rows o[16][3], r ascending (padding rows are zero)
SM_DEV float vn_rows_sum(const float *o, int c) {
    float att = 0.f;
    for (int r = 0; r < 16; ++r) att += o[r * 3 + c];
    return att;
}
// p, d of one (atom, channel): o[16][3] attention rows, wf / wd the channel's 16 weights of the rows, wfx / wdx its weight of x,
// psf / psd its shape term.  Registers or LDS: the callers hand it either.
SM_DEV void vn_linear_pd(const float *o, const float *wf, const float *wd, float wfx, float wdx, const float *x,
                         const float *psf, const float *psd, float (&p)[3], float (&d)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float xk = x[k];
        float pp = wfx * xk, dd = wdx * xk;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            pp += wf[r] * o[r * 3 + k];
            dd += wd[r] * o[r * 3 + k];
        }
        p[k] = pp + psf[k];
        d[k] = dd + psd[k];
    }
}
SM_DEV void vn_store_pd(float *out, const float (&p)[3], const float (&d)[3]) {
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; out[3] = d[0]; out[4] = d[1]; out[5] = d[2];
}
// The h2x epilogues' lane = (atom va, channel c < HD).  Its atom's rows, from this wave's LDS rows or, through L2, from the
// kernel's output (its own function: a kernel that reads either loads in two branches and shares what follows)
SM_DEV void vn_load_rows(const float *ov, float (&orow)[48]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const float4 t = ldg4(ov + 4 * i);
        orow[4 * i] = t.x; orow[4 * i + 1] = t.y; orow[4 * i + 2] = t.z; orow[4 * i + 3] = t.w;
    }
}
// ... and the rest: p and d stored, the rows' sum for a following fold (xsum, or nullptr), the lane's share of the batch sums
SM_DEV void vn_linear_atom(const VnFuse &vn, const float (&orow)[48], const float *x, float *xsum, int va, int c, int HD, double &s1, double &s2) {
    float wf[16], wd[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 t = ldg4(vn.wf_o + c * 16 + 4 * i), u = ldg4(vn.wd_o + c * 16 + 4 * i);
        wf[4 * i] = t.x; wf[4 * i + 1] = t.y; wf[4 * i + 2] = t.z; wf[4 * i + 3] = t.w;
        wd[4 * i] = u.x; wd[4 * i + 1] = u.y; wd[4 * i + 2] = u.z; wd[4 * i + 3] = u.w;
    }
    const float *psf = vn.ps + ((size_t)vn.mol_of[va] * 2 * HD + c) * 3;
    float p[3], d[3];
    vn_linear_pd(orow, wf, wd, vn.wf_x[c], vn.wd_x[c], x + va * 3, psf, psf + HD * 3, p, d);
    vn_store_pd(vn.pd + ((size_t)va * HD + c) * 6, p, d);
    if (xsum && c < 3) {
        const float a0 = vn_rows_sum(orow, 0), a1 = vn_rows_sum(orow, 1), a2 = vn_rows_sum(orow, 2);
        xsum[va * 3 + c] = c == 0 ? a0 : (c == 1 ? a1 : a2);
    }
    vn_norm_sums(p, s1, s2);
}

// ---- statistics ----------------------------------------------------------------------------------------------------
// one workgroup's sums of channel threadIdx.x into its replica
SM_DEV void vn_sums_add(double *acc, int HD, double s1, double s2) {
    acc += (size_t)(blockIdx.x % kVnReplicas) * 2 * HD;
    atomicAdd(acc + threadIdx.x, s1);
    atomicAdd(acc + HD + threadIdx.x, s2);
}
// vn_red [nwave][slots_per_wave][2]: every lane's (s1, s2), lane = 16 al + channel; waves ascending, then atoms of the wave
SM_DEV void vn_sums_commit(const double *vn_red, int slots_per_wave, int nwave, int apj, int HD, double *acc) {
    if (threadIdx.x < HD) {
        double s1 = 0.0, s2 = 0.0;
        for (int w = 0; w < nwave; ++w)
            for (int al = 0; al < apj; ++al) {
                s1 += vn_red[(w * slots_per_wave + al * 16 + threadIdx.x) * 2];
                s2 += vn_red[(w * slots_per_wave + al * 16 + threadIdx.x) * 2 + 1];
            }
        vn_sums_add(acc, HD, s1, s2);
    }
}
// total of channel c over the replicas (which = 0: sum of norms, 1: of squared norms)
SM_DEV double vn_replica_total(const double *acc, int HD, int which, int c) {
    double t = 0.0;
    for (int r = 0; r < kVnReplicas; ++r) t += acc[(size_t)r * 2 * HD + which * HD + c];
    return t;
}
// the first 32 threads of the workgroup publish the totals as sred[2][16] (16 lanes per atom = up to 16 channels)
SM_DEV void vn_stage_totals(const double *acc, int HD, double *sred) {
    if (threadIdx.x < 32) {
        const int c = threadIdx.x & 15, which = threadIdx.x >> 4;
        sred[threadIdx.x] = c < HD ? vn_replica_total(acc, HD, which, c) : 0.0;
    }
    __syncthreads();
}
// mean and 1 / sqrt(biased variance + eps) of a channel from its totals over cnt atoms
SM_DEV void vn_batch_stats(double t1, double t2, double cnt, float &meanf, float &rstd) {
    const double mean = t1 / cnt;
    double var = t2 / cnt - mean * mean;
    var = var > 0.0 ? var : 0.0;
    meanf = (float)mean;
    rstd = 1.0f / sqrtf((float)var + 1e-5f);
}

// ---- apply ---------------------------------------------------------------------------------------------------------
// batch-norm of ||p|| and VN-leaky-ReLU (slope 0.2) of one (atom, channel): pd = p (3) | d (3), g / b the channel's batch-norm
// weight and bias
SM_DEV void vn_act(const float *pd, float meanf, float rstd, float g, float b, float (&o)[3]) {
    float p[3] = {pd[0], pd[1], pd[2]};
    const float d[3] = {pd[3], pd[4], pd[5]};
    const float nrm = vn_norm(p);
    const float nbn = (nrm - meanf) * rstd * g + b;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = p[k] / nrm * nbn;
    const float dot = p[0] * d[0] + p[1] * d[1] + p[2] * d[2];
    const float dsq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const float coef = dot / (dsq + 1e-6f);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float neg = p[k] - coef * d[k];
        o[k] = 0.2f * p[k] + 0.8f * (dot >= 0.f ? p[k] : neg);
    }
}
// 16 lanes per atom, lane c = channel: the new coordinate c of atom va on lanes 0..2 (0 elsewhere)
SM_DEV float vn_update16(const float *pd, const float *x_old, const float *xsum, int va, int c, int HD,
                         float meanf, float rstd, float g, float b) {
    float o[3] = {0.f, 0.f, 0.f};
    if (c < HD) vn_act(pd + ((size_t)va * HD + c) * 6, meanf, rstd, g, b, o);
    float res[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) res[k] = seg_sum<16>(o[k]);              // over the channels of the atom
    float xn = 0.f;
    if (c < 3) {
        const float r = c == 0 ? res[0] : (c == 1 ? res[1] : res[2]);
        xn = x_old[va * 3 + c] + (xsum[va * 3 + c] / HD + r / HD);
    }
    return xn;
}
// The folded update of a workgroup: its atoms are first_atom .. last_atom; the table xt [kVnFoldCap][3] receives the new
// coordinates of the span of their molecules (-> span0, span_n), global memory those of its own atoms.  sred: 32 doubles.
SM_DEV void vn_fold_span(const VnFold &vf, int HD, int n_atoms, int first_atom, int last_atom, float *xt, double *sred, int n_threads,
                         int &span0, int &span_n) {
    if (first_atom <= last_atom) {
        span0 = vf.mol_span[first_atom].x;
        const int span = vf.mol_span[last_atom].y - span0;
        if (span > kVnFoldCap && threadIdx.x == 0) *vf.span_flag = 1;      // the max_mol_atoms hint was too small
        span_n = min(span, kVnFoldCap);
    }
    vn_stage_totals(vf.acc, HD, sred);
    const int c = threadIdx.x & 15;
    float meanf = 0.f, rstd = 0.f, bng = 0.f, bnb = 0.f;
    if (c < HD) {
        vn_batch_stats(sred[c], sred[16 + c], (double)n_atoms, meanf, rstd);
        bng = vf.bn_g[c]; bnb = vf.bn_b[c];
    }
    for (int it = threadIdx.x; it < span_n * 16; it += n_threads) {         // item = (atom of the span, channel)
        const int va = span0 + (it >> 4);
        const float xn = vn_update16(vf.pd, vf.x_old, vf.xsum, va, c, HD, meanf, rstd, bng, bnb);
        if (c < 3) {
            xt[(it >> 4) * 3 + c] = xn;
            if (va >= first_atom && va <= last_atom) vf.x_new[va * 3 + c] = xn;
        }
    }
}
