// Training the shape decoder: the loss's gradient with respect to every decoder parameter, the latent z and the query points,
// deterministic (no atomics; every sum over points and shapes in a fixed order, float64 where partials meet).
//
// Phase one, sd_train_kernel: sd_sweep (sm_shape_dec_grad.h), the very body sd_grad_kernel runs (so the value is the decode
// kernel's bit for bit), with the upstream gradient u at the top (times s (1 - s) for occupancy) -- and on the way its taps STORE
// what the sweep otherwise throws away, per point of the chunk:
//     slot i          (i < 2 L)   the ReLU'd operand of Linear i            A_i  = relu(x) (i even), relu(net) (i odd)
//     slot 2 L + i    (i < 2 L)   the upstream gradient of Linear i's output dY_i = g_y (i even), g (i odd)
//     slot 4 L                    g at fc_in's output (after the last block backwards)
//     slot 4 L + 1                u' relu(x_L)   (whose column sum is dw_out)
// and u' itself in up[chunk].  A slot is stored in the kernel's own fragment order, [16-point group][t][lane][r]: the f32x4 a
// lane holds (rows 16 t + 4 g + r of point n, lane = 16 g + n) goes out as it is, so a store instruction of a wave writes 1 KB
// contiguous.  Row-major [point][128] would turn the same store into 16 pieces of 64 bytes.  The order of the points inside a
// slot is free, since phase two sums over them and both operands of a product share it.
// Tail lanes of the last tile compute the last point again with u' = 0: every gradient they store is zero.
//
// Phase two, sd_dw_kernel: dW_i = dY_i^T A_i, a 128 x 128 x K product with K the chunk's points, split over K.  A workgroup
// takes one Linear and a range of 16-point groups; a group of each operand (8 KB, contiguous) goes through LDS as [point][row],
// from where the matrix cores take dY as the A operand (lane = row, k = point) and A as the B operand.  The column sums of dY
// (the bias gradient) fall out of the same LDS tile.  Partials [Linear][split] are added by sd_dw_reduce_kernel in split
// order into float64 accumulators that persist across the chunks of a call (chunk order).
//
// fc_in and the prologue: sd_shape_sums_kernel adds, per shape, g (x) p, g, g |p|^2, u' relu(x_L) and u' over the shape's points
// of the chunk (float64, fixed order).  After the last chunk sd_prologue_back_kernel (one workgroup per shape) turns a shape's
// sums dG_b, dc_b into dz_b, and sd_head_weights_kernel gives every element of z_in, fc_in and fc_out one thread that walks the
// shapes in shape order -- the fixed-order reduction over shapes without a [shape][weight] buffer (65535 shapes x 131 K
// weights would not fit anywhere).
#pragma once
#include "sm_shape_dec_grad.h"

constexpr int kSdTrainTile = kSdGradTile;                  // points per workgroup iteration: sd_grad_kernel's 4 waves x 2 column tiles
constexpr int kSdGroup = 16 * kSdH;                        // floats of a 16-point group of one slot
constexpr int kSdSums = 7;                                 // per shape and hidden unit: G_x G_y G_z c |p|^2 e u
constexpr int kSdMaxSplits = 64;

SM_DEV void sd_store_frag(float *slot, int64_t grp, int lane, const f32x4 (&x)[8], bool relu) {
    float *dst = slot + grp * kSdGroup + lane * 4;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const f32x4 v = x[t];
        stg4(dst + t * 256, relu ? make_float4(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f))
                                 : make_float4(v[0], v[1], v[2], v[3]));
    }
}

struct SdTrainArgs {
    SdArgs d;                // the chunk's points: d.p, d.out already offset; d.n = points of the chunk
    int64_t first;           // index of the chunk's first point in the whole launch (its shape is (first + i) / per_shape)
    const float *up_in;      // [n] upstream gradient (offset)
    float *grad;             // [n][3] (offset) or null
    float *slots;            // [4 L + 2][cap * 128]
    float *up;               // [cap]
    int64_t cap;             // points a slot holds (whole tiles)

    // sd_sweep's Mode (sm_shape_dec_grad.h)
    static constexpr bool kTaps = true;
    SM_DEV int64_t point(int64_t pt, float &px, float &py, float &pz) const {
        const int64_t q = pt < d.n ? pt : d.n - 1;
        px = d.p[q * 3]; py = d.p[q * 3 + 1]; pz = d.p[q * 3 + 2];
        const int64_t s = (first + q) / d.per_shape;
        return s >= d.B ? d.B - 1 : s;
    }
    // u' = u (times s (1 - s)), kept in up[]; tail lanes of the last tile take u = 0
    SM_DEV float top(int g, int64_t pt, float val) const {
        const float u = pt < d.n ? up_in[pt] : 0.f;
        const float uf = d.sigmoid ? u * (val * (1.f - val)) : u;
        if (g == 0) up[pt] = uf;
        return uf;
    }
    SM_DEV void tap(int slot, int64_t grp, int lane, const f32x4 (&x)[8], bool relu) const {
        sd_store_frag(slots + (size_t)slot * ((size_t)cap * kSdH), grp, lane, x, relu);
    }
    SM_DEV void epilogue(int64_t, int64_t, float, float, float, float, float, float, float) const {}
};

__global__ void __launch_bounds__(kSdGradWaves * 64) sd_train_kernel(SdTrainArgs ta) { sd_sweep(ta.d, ta); }

// ---- phase two: dW_i = dY_i^T A_i over the chunk's groups, split over the groups ------------------------------------------------
// grid (2 L, splits), 256 threads.  Wave w owns output row tiles 2 w, 2 w + 1 and all eight column tiles.
// pw [2 L][splits][128 * 128] float, pb [2 L][splits][128] double.
constexpr int kSdDwLd = kSdH + 16;                         // LDS row of a point: the four points a k-step reads lie 16 banks apart
__global__ void __launch_bounds__(256) sd_dw_kernel(const float *slots, size_t slot_sz, int L, int64_t n_groups, int per_split, float *pw, double *pb) {
    __shared__ __attribute__((aligned(16))) float ds[16 * kSdDwLd], as[16 * kSdDwLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int lin = blockIdx.x, split = blockIdx.y, splits = gridDim.y;
    const float *A = slots + (size_t)lin * slot_sz, *D = slots + (size_t)(2 * L + lin) * slot_sz;
    const int64_t g0 = (int64_t)split * per_split, g1 = g0 + per_split < n_groups ? g0 + per_split : n_groups;
    f32x4 acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    double bsum = 0.0;
    // float4 e of a group (e = tid, tid + 256): t = e / 64, lane' = e % 64 -> point lane' & 15, rows 16 t + 4 (lane' >> 4) ..
    float4 rd[2], ra[2];
    auto fetch = [&](int64_t grp) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            rd[h] = ldg4(D + grp * kSdGroup + (tid + 256 * h) * 4);
            ra[h] = ldg4(A + grp * kSdGroup + (tid + 256 * h) * 4);
        }
    };
    if (g0 < g1) fetch(g0);
    for (int64_t grp = g0; grp < g1; ++grp) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = tid + 256 * h, t = e >> 6, l2 = e & 63;
            const int o = (l2 & 15) * kSdDwLd + 16 * t + 4 * (l2 >> 4);
            *reinterpret_cast<float4 *>(ds + o) = rd[h];
            *reinterpret_cast<float4 *>(as + o) = ra[h];
        }
        __syncthreads();
        if (grp + 1 < g1) fetch(grp + 1);
        if (tid < kSdH) {
#pragma unroll
            for (int k = 0; k < 16; ++k) bsum += (double)ds[k * kSdDwLd + tid];
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const float a0 = ds[(4 * kk + lk) * kSdDwLd + 32 * wave + li], a1 = ds[(4 * kk + lk) * kSdDwLd + 32 * wave + 16 + li];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float bv = as[(4 * kk + lk) * kSdDwLd + 16 * j + li];
                acc[0][j] = mfma16(a0, bv, acc[0][j]);
                acc[1][j] = mfma16(a1, bv, acc[1][j]);
            }
        }
        __syncthreads();
    }
    float *C = pw + ((size_t)lin * splits + split) * kSdImg;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) C[(size_t)(32 * wave + 16 * i + 4 * lk + r) * kSdH + 16 * j + li] = acc[i][j][r];
    if (tid < kSdH) pb[((size_t)lin * splits + split) * kSdH + tid] = bsum;
}

// accW [2 L][128 * 128 + 128] double (+)= the partials of a chunk, split order; first: the chunk is the call's first
__global__ void __launch_bounds__(256) sd_dw_reduce_kernel(const float *pw, const double *pb, int splits, int first, double *accW) {
    const int lin = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kSdImg + kSdH) return;
    double s = 0.0;
    if (i < kSdImg) for (int k = 0; k < splits; ++k) s += (double)pw[((size_t)lin * splits + k) * kSdImg + i];
    else for (int k = 0; k < splits; ++k) s += pb[((size_t)lin * splits + k) * kSdH + (i - kSdImg)];
    double *dst = accW + (size_t)lin * (kSdImg + kSdH) + i;
    *dst = first ? s : *dst + s;
}

// ---- per-shape sums over the chunk's points: accS [B][kSdSums][128] double ----------------------------------------------------------
// One workgroup per shape, 512 threads = (t, lane) of a group's float4s; the 16 points of a group are added in point order.
__global__ void __launch_bounds__(512) sd_shape_sums_kernel(const float *slots, size_t slot_sz, int L, const float *up, const float *p /* chunk */,
                                                            int64_t first, int64_t n, int64_t per_shape, int is_first, double *accS) {
    __shared__ double red[512][4];
    const int b = blockIdx.x, tid = threadIdx.x, t = tid >> 6, lane = tid & 63, nn = lane & 15, gq = lane >> 4;
    const float *G = slots + (size_t)(4 * L) * slot_sz, *E = slots + (size_t)(4 * L + 1) * slot_sz;
    // the shape's points inside the chunk, as chunk-local indices [lo, hi)
    int64_t lo = (int64_t)b * per_shape - first, hi = lo + per_shape;
    lo = lo < 0 ? 0 : lo; hi = hi > n ? n : hi;
    double s[kSdSums - 1][4], su = 0.0;
#pragma unroll
    for (int q = 0; q < kSdSums - 1; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[q][r] = 0.0;
    if (lo < hi) {
        for (int64_t grp = lo / 16; grp * 16 < hi; ++grp) {
            const int64_t pt = grp * 16 + nn;
            if (pt < lo || pt >= hi) continue;
            const float4 gv = ldg4(G + grp * kSdGroup + tid * 4), ev = ldg4(E + grp * kSdGroup + tid * 4);
            const double x = p[pt * 3], y = p[pt * 3 + 1], z = p[pt * 3 + 2], pp = (double)(p[pt * 3] * p[pt * 3] + p[pt * 3 + 1] * p[pt * 3 + 1] + p[pt * 3 + 2] * p[pt * 3 + 2]);
            const float gr[4] = {gv.x, gv.y, gv.z, gv.w}, er[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double gd = gr[r];
                s[0][r] += gd * x; s[1][r] += gd * y; s[2][r] += gd * z; s[3][r] += gd; s[4][r] += gd * pp; s[5][r] += (double)er[r];
            }
            su += (double)up[pt];
        }
    }
    double *dst = accS + (size_t)b * kSdSums * kSdH;
#pragma unroll
    for (int q = 0; q < kSdSums; ++q) {                                        // (unrolled: s[q] stays in registers)
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) red[tid][r] = q < kSdSums - 1 ? s[q < kSdSums - 1 ? q : 0][r] : su;
        __syncthreads();
        if (nn == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double v = 0.0;
                for (int k = 0; k < 16; ++k) v += red[tid + k][r];
                double *d = dst + q * kSdH + 16 * t + 4 * gq + r;
                *d = is_first ? v : *d + v;
            }
        }
    }
}

// ---- prologue backwards, per shape: dz_b and dz_inv,b from the shape's dG_b, dc_b ---------------------------------------------------
// dz_inv = Winv^T dc;  dz_dir = dz_inv (.) z;  dz = Wz^T dG + dz_inv (.) z_dir + W_zin^T dz_dir     (plain fp32 FMAs, as the prologue)
__global__ void __launch_bounds__(256) sd_prologue_back_kernel(const float *z, const float *w_zin, const float *w_in, int Z, const double *accS,
                                                               float *dzinv, float *grad_z) {
    __shared__ float zs[256 * 3], dgs[kSdH * 4], dzi[256];
    const int b = blockIdx.x;
    const float *zb = z + (size_t)b * Z * 3;
    const double *sb = accS + (size_t)b * kSdSums * kSdH;
    for (int e = threadIdx.x; e < Z * 3; e += blockDim.x) zs[e] = zb[e];
    for (int e = threadIdx.x; e < kSdH * 4; e += blockDim.x) dgs[e] = (float)sb[(e & 3) * kSdH + (e >> 2)];      // [h][x y z c]
    __syncthreads();
    const int ld = 2 * Z + 1;
    for (int m = threadIdx.x; m < Z; m += blockDim.x) {
        float v = 0.f;
        for (int h = 0; h < kSdH; ++h) v = fmaf(w_in[(size_t)h * ld + 1 + Z + m], dgs[h * 4 + 3], v);
        dzi[m] = v;
        dzinv[(size_t)b * Z + m] = v;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < Z; m += blockDim.x) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        for (int h = 0; h < kSdH; ++h) {
            const float w = w_in[(size_t)h * ld + 1 + m];
            gx = fmaf(w, dgs[h * 4], gx); gy = fmaf(w, dgs[h * 4 + 1], gy); gz = fmaf(w, dgs[h * 4 + 2], gz);
        }
        float dx = 0.f, dy = 0.f, dz = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
        for (int k = 0; k < Z; ++k) {
            const float w = w_zin[(size_t)m * Z + k];                          // z_dir[m] = sum_k W[m][k] z[k]
            dx = fmaf(w, zs[3 * k], dx); dy = fmaf(w, zs[3 * k + 1], dy); dz = fmaf(w, zs[3 * k + 2], dz);
            const float wt = w_zin[(size_t)k * Z + m] * dzi[k];                // W^T dz_dir, dz_dir[k] = dz_inv[k] z[k]
            tx = fmaf(wt, zs[3 * k], tx); ty = fmaf(wt, zs[3 * k + 1], ty); tz = fmaf(wt, zs[3 * k + 2], tz);
        }
        float *o = grad_z + ((size_t)b * Z + m) * 3;
        o[0] = gx + fmaf(dzi[m], dx, tx); o[1] = gy + fmaf(dzi[m], dy, ty); o[2] = gz + fmaf(dzi[m], dz, tz);
    }
}

// ---- the gradients of z_in, fc_in and fc_out: one thread per element, the shapes in shape order (float64) ---------------------------
// gw: the gradient vector in the weights' order; elements [0, Z Z) z_in, then fc_in.weight [H][2 Z + 1], fc_in.bias [H]; o_out:
// offset of fc_out.weight [H] and fc_out.bias
__global__ void __launch_bounds__(256) sd_head_weights_kernel(const float *z, const float *zinv, const float *dzinv, const double *accS, int Z, int B,
                                                              size_t o_out, float *gw) {
    const int ld = 2 * Z + 1;
    const int64_t n_zin = (int64_t)Z * Z, n_win = (int64_t)kSdH * ld, total = n_zin + n_win + kSdH + kSdH + 1;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    double s = 0.0;
    const size_t ss = (size_t)kSdSums * kSdH;
    if (i < n_zin) {                                                           // dW_zin[m][k] = sum_b dz_inv[m] (z[m] . z[k])
        const int m = (int)(i / Z), k = (int)(i % Z);
        for (int b = 0; b < B; ++b) {
            const float *zb = z + (size_t)b * Z * 3;
            s += (double)dzinv[(size_t)b * Z + m] * ((double)zb[3 * m] * zb[3 * k] + (double)zb[3 * m + 1] * zb[3 * k + 1] + (double)zb[3 * m + 2] * zb[3 * k + 2]);
        }
        gw[i] = (float)s;
    } else if (i < n_zin + n_win) {
        const int64_t e = i - n_zin;
        const int h = (int)(e / ld), c = (int)(e % ld);
        if (c == 0) for (int b = 0; b < B; ++b) s += accS[b * ss + 4 * kSdH + h];
        else if (c <= Z) {
            const int m = c - 1;
            for (int b = 0; b < B; ++b) {
                const float *zm = z + ((size_t)b * Z + m) * 3;
                s += accS[b * ss + h] * zm[0] + accS[b * ss + kSdH + h] * zm[1] + accS[b * ss + 2 * kSdH + h] * zm[2];
            }
        } else {
            const int m = c - 1 - Z;
            for (int b = 0; b < B; ++b) s += accS[b * ss + 3 * kSdH + h] * (double)zinv[(size_t)b * Z + m];
        }
        gw[i] = (float)s;
    } else if (i < n_zin + n_win + kSdH) {
        const int h = (int)(i - n_zin - n_win);
        for (int b = 0; b < B; ++b) s += accS[b * ss + 3 * kSdH + h];
        gw[i] = (float)s;
    } else {
        const int h = (int)(i - n_zin - n_win - kSdH);                         // h == H: fc_out.bias
        for (int b = 0; b < B; ++b) s += h < kSdH ? accS[b * ss + 5 * kSdH + h] : accS[b * ss + 6 * kSdH];
        gw[o_out + h] = (float)s;
    }
}

// the blocks' gradients from the float64 accumulators: Linear i -> gw + o_blocks + i (H H + H): weight [H][H], bias [H]
__global__ void __launch_bounds__(256) sd_dw_finish_kernel(const double *accW, float *gw_blocks) {
    const int lin = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kSdImg + kSdH) return;
    gw_blocks[(size_t)lin * (kSdImg + kSdH) + i] = (float)accW[(size_t)lin * (kSdImg + kSdH) + i];
}
