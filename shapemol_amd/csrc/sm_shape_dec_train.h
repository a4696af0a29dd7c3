// Training the shape decoder: the loss's gradient with respect to every decoder parameter, the latent z and the query points,
// deterministic (no atomics; every sum over points and shapes in a fixed order, float64 where partials meet).
//
// Phase one, sd_train_kernel: sd_grad_kernel's forward and reverse sweep, call for call (so the value is the decode kernel's bit
// for bit), with the upstream gradient u at the top (times s (1 - s) for occupancy) -- and on the way it STORES what the sweep
// otherwise throws away, per point of the chunk:
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

struct SdTrainArgs {
    SdArgs d;                // the chunk's points: d.p, d.out already offset; d.n = points of the chunk
    int64_t first;           // index of the chunk's first point in the whole launch (its shape is (first + i) / per_shape)
    const float *up_in;      // [n] upstream gradient (offset)
    float *grad;             // [n][3] (offset) or null
    float *slots;            // [4 L + 2][cap * 128]
    float *up;               // [cap]
    int64_t cap;             // points a slot holds (whole tiles)
};

SM_DEV void sd_store_frag(float *slot, int64_t grp, int lane, const f32x4 (&x)[8], bool relu) {
    float *dst = slot + grp * kSdGroup + lane * 4;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const f32x4 v = x[t];
        stg4(dst + t * 256, relu ? make_float4(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f))
                                 : make_float4(v[0], v[1], v[2], v[3]));
    }
}

__global__ void __launch_bounds__(kSdGradWaves * 64) sd_train_kernel(SdTrainArgs ta) {
    const SdArgs &a = ta.d;
    extern __shared__ float wl[];                          // [2][kSdImg]; [2 L][H] biases
    float *bl = wl + 2 * kSdImg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int64_t n_tiles = (a.n + kSdTrainTile - 1) / kSdTrainTile;
    const int n_lin = 2 * a.L, n_img = 4 * a.L;
    const size_t slot_sz = (size_t)ta.cap * kSdH;
    if ((int64_t)blockIdx.x < n_tiles) dma_to_lds(wl, a.img, kSdImg / 4, wave, kSdGradWaves, lane);
    for (int e = threadIdx.x; e < n_lin * kSdH; e += kSdGradWaves * 64) bl[e] = a.bias[e];
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const bool last_tile = tile + gridDim.x >= n_tiles;
        f32x4 x[kSdGradColTiles][8], y[kSdGradColTiles][8];
        unsigned mk[kSdGradColTiles][kSdMasks];
        int64_t pt[kSdGradColTiles], sb[kSdGradColTiles], grp[kSdGradColTiles];
        float px[kSdGradColTiles], py[kSdGradColTiles], pz[kSdGradColTiles];
#pragma unroll
        for (int ct = 0; ct < kSdGradColTiles; ++ct) {
#pragma unroll
            for (int k = 0; k < kSdMasks; ++k) mk[ct][k] = 0;
            grp[ct] = tile * (kSdTrainTile / 16) + wave * kSdGradColTiles + ct;
            pt[ct] = grp[ct] * 16 + n;
            const int64_t q = pt[ct] < a.n ? pt[ct] : a.n - 1;
            px[ct] = a.p[q * 3]; py[ct] = a.p[q * 3 + 1]; pz[ct] = a.p[q * 3 + 2];
            const int64_t s = (ta.first + q) / a.per_shape;
            sb[ct] = s >= a.B ? a.B - 1 : s;
            sd_fc_in(a, sb[ct], g, px[ct], py[ct], pz[ct], x[ct]);
        }
        // ---- forward, as sd_grad_kernel; the operands of both Linears of a block go out as they are formed
        for (int i = 0; i < n_lin; i += 2) {
            sd_image_barrier();
            dma_to_lds(wl + kSdImg, a.img + (size_t)(i + 1) * kSdImg, kSdImg / 4, wave, kSdGradWaves, lane);
#pragma unroll
            for (int ct = 0; ct < kSdGradColTiles; ++ct) {
                sd_mask_put(mk[ct], i, sd_relu_mask(x[ct]));
                sd_store_frag(ta.slots + (size_t)i * slot_sz, grp[ct], lane, x[ct], true);
            }
            sd_bias(bl + i * kSdH, g, y);
            sd_linear(wl, lane, x, y);
            sd_image_barrier();
            dma_to_lds(wl, a.img + (size_t)(i + 2) * kSdImg, kSdImg / 4, wave, kSdGradWaves, lane);
#pragma unroll
            for (int ct = 0; ct < kSdGradColTiles; ++ct) {
                sd_mask_put(mk[ct], i + 1, sd_relu_mask(y[ct]));
                sd_store_frag(ta.slots + (size_t)(i + 1) * slot_sz, grp[ct], lane, y[ct], true);
            }
            sd_linear_residual(wl + kSdImg, bl + (i + 1) * kSdH, lane, g, y, x);
        }
        // ---- fc_out and its way back: g = u' w_out (.) m_last, u' = u (times s (1 - s)); slot 4 L + 1 takes u' relu(x_L)
        float val[kSdGradColTiles];
#pragma unroll
        for (int ct = 0; ct < kSdGradColTiles; ++ct) {
            val[ct] = sd_fc_out(a, g, x[ct]);
            const unsigned m = sd_relu_mask(x[ct]);
            const float u = pt[ct] < a.n ? ta.up_in[pt[ct]] : 0.f;
            const float uf = a.sigmoid ? u * (val[ct] * (1.f - val[ct])) : u;
            if (g == 0) ta.up[pt[ct]] = uf;
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) y[ct][t][r] = uf * fmaxf(x[ct][t][r], 0.f);
            sd_store_frag(ta.slots + (size_t)(n_img + 1) * slot_sz, grp[ct], lane, y[ct], false);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float4 w = ldg4(a.w_out + 16 * t + 4 * g);
                x[ct][t] = f32x4{w.x * uf, w.y * uf, w.z * uf, w.w * uf};
            }
            sd_mask_apply(m, x[ct]);
        }
        // ---- backward through the blocks: dY of fc_1 (g) and of fc_0 (g_y) go out
        for (int j = n_lin; j < n_img; j += 2) {
            const int b = (n_img - 2 - j) >> 1;
            sd_image_barrier();
            dma_to_lds(wl + kSdImg, a.img + (size_t)(j + 1) * kSdImg, kSdImg / 4, wave, kSdGradWaves, lane);
#pragma unroll
            for (int ct = 0; ct < kSdGradColTiles; ++ct) {
                sd_store_frag(ta.slots + (size_t)(n_lin + 2 * b + 1) * slot_sz, grp[ct], lane, x[ct], false);
#pragma unroll
                for (int t = 0; t < 8; ++t) y[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            sd_linear<false>(wl, lane, x, y);
            unsigned mx[kSdGradColTiles];
#pragma unroll
            for (int ct = 0; ct < kSdGradColTiles; ++ct) {
                sd_mask_apply(sd_mask_get(mk[ct], 2 * b + 1), y[ct]);
                mx[ct] = sd_mask_get(mk[ct], 2 * b);
                sd_store_frag(ta.slots + (size_t)(n_lin + 2 * b) * slot_sz, grp[ct], lane, y[ct], false);
            }
            sd_image_barrier();
            if (j + 2 < n_img || !last_tile)
                dma_to_lds(wl, a.img + (size_t)(j + 2 < n_img ? j + 2 : 0) * kSdImg, kSdImg / 4, wave, kSdGradWaves, lane);
            sd_linear_back_residual(wl + kSdImg, lane, y, mx, x);
        }
        // ---- fc_in backwards: g goes out; grad_p = 2 p (w0 . g) + G^T g
#pragma unroll
        for (int ct = 0; ct < kSdGradColTiles; ++ct) {
            sd_store_frag(ta.slots + (size_t)n_img * slot_sz, grp[ct], lane, x[ct], false);
            const float *gcb = a.gc + sb[ct] * (kSdH * 4);
            float s0 = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float4 w0 = ldg4(a.w0 + 16 * t + 4 * g);
                const float w0r[4] = {w0.x, w0.y, w0.z, w0.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float4 gc = ldg4(gcb + (16 * t + 4 * g + r) * 4);
                    const float gv = x[ct][t][r];
                    s0 = fmaf(w0r[r], gv, s0); sx = fmaf(gc.x, gv, sx); sy = fmaf(gc.y, gv, sy); sz = fmaf(gc.z, gv, sz);
                }
            }
            s0 += __shfl_xor(s0, 16, 64); sx += __shfl_xor(sx, 16, 64); sy += __shfl_xor(sy, 16, 64); sz += __shfl_xor(sz, 16, 64);
            s0 += __shfl_xor(s0, 32, 64); sx += __shfl_xor(sx, 32, 64); sy += __shfl_xor(sy, 32, 64); sz += __shfl_xor(sz, 32, 64);
            if (g != 0 || pt[ct] >= a.n) continue;
            const int64_t q = pt[ct];
            if (a.out) a.out[q] = val[ct];
            if (ta.grad) {
                ta.grad[q * 3] = fmaf(2.f * px[ct], s0, sx); ta.grad[q * 3 + 1] = fmaf(2.f * py[ct], s0, sy); ta.grad[q * 3 + 2] = fmaf(2.f * pz[ct], s0, sz);
            }
        }
    }
}

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

// ---- weights from device memory: the context's images from one flat vector in the host packing's order ---------------------------
struct SdRepackArgs {
    const float *w;          // z_in | fc_in.weight | fc_in.bias | 2 L x (weight, bias) | fc_out.weight, fc_out.bias
    float *dst;              // the context's block
    size_t o_zin, o_win, o_bin, o_w0, o_img, o_bias, o_out;
    int Z, L;
};
// grid (x, 1 + 2 L): y == 0 the head and tail pieces, y == 1 + i Linear i (forward image i, transposed image 4 L - 1 - i, bias i)
__global__ void __launch_bounds__(256) sd_repack_kernel(SdRepackArgs a) {
    const int Z = a.Z, ld = 2 * Z + 1;
    const size_t n_zin = (size_t)Z * Z, n_win = (size_t)kSdH * ld, o_lin = n_zin + n_win + kSdH;
    if (blockIdx.y == 0) {
        const size_t total = n_zin + n_win + kSdH + kSdH + (kSdH + 1);
        for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
            if (e < n_zin) a.dst[a.o_zin + e] = a.w[e];
            else if (e < n_zin + n_win) a.dst[a.o_win + (e - n_zin)] = a.w[e];
            else if (e < o_lin) a.dst[a.o_bin + (e - n_zin - n_win)] = a.w[e];
            else if (e < o_lin + kSdH) a.dst[a.o_w0 + (e - o_lin)] = a.w[n_zin + (e - o_lin) * ld];
            else a.dst[a.o_out + (e - o_lin - kSdH)] = a.w[o_lin + (size_t)2 * a.L * (kSdImg + kSdH) + (e - o_lin - kSdH)];
        }
        return;
    }
    const int i = blockIdx.y - 1;
    const float *W = a.w + o_lin + (size_t)i * (kSdImg + kSdH);
    float *fw = a.dst + a.o_img + (size_t)i * kSdImg, *bw = a.dst + a.o_img + (size_t)(4 * a.L - 1 - i) * kSdImg;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < kSdImg + kSdH; e += gridDim.x * 256) {
        if (e >= kSdImg) { a.dst[a.o_bias + (size_t)i * kSdH + (e - kSdImg)] = W[e]; continue; }
        const int r = e & 3, lane = (e >> 2) & 63, ti = (e >> 8) & 7, to = e >> 11;
        const int row = 16 * to + (lane & 15), col = 16 * ti + 4 * (lane >> 4) + r;
        fw[e] = W[row * kSdH + col];
        bw[e] = W[col * kSdH + row];
    }
}
