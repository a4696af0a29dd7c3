// Shape decoder on the device: DecoderInner.forward of the reference's shape auto-encoder
// (models/shape_pointcloud_modelAE.py:69-103 with ResnetBlockFC, models/shape_vn_layers.py:210-252): the implicit field
// (signed distance or occupancy) of a shape latent z (Z, 3) at query points p.
//
// Formulation.  The reference feeds fc_in the 2Z+1 features [ |p|^2 , p.z_0 .. p.z_{Z-1} , z_inv ].  Only |p|^2 and p depend on
// the point, so with W = fc_in.weight split by columns as [w0 | Wz | Winv]
//     fc_in(feature) = w0 |p|^2 + G_b p + c_b,      G_b [H][3] = Wz z_b,   c_b [H] = Winv z_inv,b + bias
// G and c are built once per shape (sd_prologue_kernel) and a point costs four FMAs per hidden unit instead of 2Z+1.
//
// sd_decode_kernel takes kSdTile points per workgroup iteration through fc_in, every residual block and fc_out without leaving
// the registers.  A column of the products is a point; a wave owns kSdColTiles tiles of 16 columns.  Y = W X runs on the exact
// fp32-input matrix cores (v_mfma_f32_16x16x4_f32): the accumulator of row tile t holds rows 16 t + 4 g + r of column n in lane
// (n, g), register r -- exactly the B operand of a k-step whose four k indices are 16 t + 4 g + r (g = 0..3).  So a layer's output
// is the next layer's operand with no lane movement, provided the weight image lists its k in that order:
//     wimg[((to * 8 + ti) * 64 + lane) * 4 + r] = W[16 to + (lane & 15)][16 ti + 4 (lane >> 4) + r]
// The 64 KB image of a Linear is shared by the workgroup's waves through LDS (ds_read_b128, one per 4 k-steps and kSdColTiles
// column tiles).  Two image buffers: while the waves multiply by image i, LDS-DMA (dma_to_lds) brings image i + 1, the first
// image of the workgroup's next tile included, so one barrier per Linear is all the synchronisation there is.
// Columns are independent: every output is a fixed-order fp32 fma chain over its own column, whatever else shares the tile.
#pragma once
#include "sm_device.h"

constexpr int kSdH = 128;                                  // hidden_size (checked on the host)
constexpr int kSdColTiles = 2;                             // 16-column tiles per wave
constexpr int kSdWaves = 8;
constexpr int kSdTile = kSdWaves * kSdColTiles * 16;       // points per workgroup iteration
constexpr int kSdImg = kSdH * kSdH;                        // floats of one Linear's image

// ---- per-shape prologue: z_dir = z_in(z), z_inv = sum_xyz z * z_dir, G = Wz z, c = Winv z_inv + bias ---------------------------
// One workgroup per shape.  gc [B][H][4] = (G_x, G_y, G_z, c) per hidden unit; zinv [B][Z].
__global__ void __launch_bounds__(256) sd_prologue_kernel(const float *z, const float *w_zin, const float *w_in, const float *b_in,
                                                          int Z, float *zinv, float *gc) {
    __shared__ float zs[256 * 3], zi[256];
    const int b = blockIdx.x;
    const float *zb = z + (size_t)b * Z * 3;
    for (int e = threadIdx.x; e < Z * 3; e += blockDim.x) zs[e] = zb[e];
    __syncthreads();
    for (int m = threadIdx.x; m < Z; m += blockDim.x) {
        float dx = 0.f, dy = 0.f, dz = 0.f;
        for (int k = 0; k < Z; ++k) {
            const float w = w_zin[(size_t)m * Z + k];
            dx = fmaf(w, zs[3 * k], dx); dy = fmaf(w, zs[3 * k + 1], dy); dz = fmaf(w, zs[3 * k + 2], dz);
        }
        const float v = zs[3 * m] * dx + zs[3 * m + 1] * dy + zs[3 * m + 2] * dz;
        zi[m] = v;
        zinv[(size_t)b * Z + m] = v;
    }
    __syncthreads();
    const int ld = 2 * Z + 1;
    for (int h = threadIdx.x; h < kSdH; h += blockDim.x) {
        const float *wz = w_in + (size_t)h * ld + 1, *wi = wz + Z;
        float gx = 0.f, gy = 0.f, gz = 0.f, c = 0.f;
        for (int m = 0; m < Z; ++m) {
            const float w = wz[m];
            gx = fmaf(w, zs[3 * m], gx); gy = fmaf(w, zs[3 * m + 1], gy); gz = fmaf(w, zs[3 * m + 2], gz);
            c = fmaf(wi[m], zi[m], c);
        }
        stg4(gc + ((size_t)b * kSdH + h) * 4, make_float4(gx, gy, gz, c + b_in[h]));
    }
}

// ---- fused decode -----------------------------------------------------------------------------------------------------------
struct SdArgs {
    const float *p;          // [n][3]
    const int *shape_of;     // [n] or null: shape of point i is i / per_shape
    const float *gc;         // [B][H][4]
    const float *w0;         // [H] column 0 of fc_in.weight (|p|^2)
    const float *img;        // [2 L] images of fc_0 / fc_1 of every block
    const float *bias;       // [2 L][H]
    const float *w_out;      // [H] fc_out.weight, then fc_out.bias
    float *out;              // [n]
    int64_t n, per_shape;    // n < 2^31 (host)
    int B, L, sigmoid;
};

// point `pt` of the launch (clamped into [0, n): tails compute the last point again and store nothing) and the shape it
// belongs to (clamped into [0, B))
SM_DEV int64_t sd_point(const SdArgs &a, int64_t pt, float &px, float &py, float &pz) {
    const int64_t q = pt < a.n ? pt : a.n - 1;
    px = a.p[q * 3]; py = a.p[q * 3 + 1]; pz = a.p[q * 3 + 2];
    const int64_t sb = a.shape_of ? (int64_t)a.shape_of[q] : q / a.per_shape;
    return sb < 0 ? 0 : (sb >= a.B ? a.B - 1 : sb);
}

// fc_in of one column: rows 16 t + 4 g + r of w0 |p|^2 + G_sb p + c_sb
SM_DEV void sd_fc_in(const SdArgs &a, int64_t sb, int g, float px, float py, float pz, f32x4 (&x)[8]) {
    const float pp = px * px + py * py + pz * pz;
    const float *gcb = a.gc + sb * (kSdH * 4);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const float4 w0 = ldg4(a.w0 + 16 * t + 4 * g);
        const float w0r[4] = {w0.x, w0.y, w0.z, w0.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4 gc = ldg4(gcb + (16 * t + 4 * g + r) * 4);
            x[t][r] = fmaf(w0r[r], pp, fmaf(gc.x, px, fmaf(gc.y, py, fmaf(gc.z, pz, gc.w))));
        }
    }
}

// fc_out(relu(x)) of one column: this lane's 32 rows, then the four lane groups of the column; sigmoid for occupancy
SM_DEV float sd_fc_out(const SdArgs &a, int g, const f32x4 (&x)[8]) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const float4 w = ldg4(a.w_out + 16 * t + 4 * g);
        s = fmaf(w.x, fmaxf(x[t][0], 0.f), s); s = fmaf(w.y, fmaxf(x[t][1], 0.f), s);
        s = fmaf(w.z, fmaxf(x[t][2], 0.f), s); s = fmaf(w.w, fmaxf(x[t][3], 0.f), s);
    }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    s += a.w_out[kSdH];
    if (a.sigmoid) s = 1.f / (1.f + expf(-s));
    return s;
}

// fc_in backwards of one column, sd_fc_in's sibling: with x the gradient at fc_in's output, d/dp = 2 p (w0 . x) + G_sb^T x over the
// column's 128 rows -- this lane's 32, then the four lane groups of the column
SM_DEV void sd_fc_in_back(const SdArgs &a, int64_t sb, int g, float px, float py, float pz, const f32x4 (&x)[8], float &gx, float &gy, float &gz) {
    const float *gcb = a.gc + sb * (kSdH * 4);
    float s0 = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const float4 w0 = ldg4(a.w0 + 16 * t + 4 * g);
        const float w0r[4] = {w0.x, w0.y, w0.z, w0.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4 gc = ldg4(gcb + (16 * t + 4 * g + r) * 4);
            const float gv = x[t][r];
            s0 = fmaf(w0r[r], gv, s0); sx = fmaf(gc.x, gv, sx); sy = fmaf(gc.y, gv, sy); sz = fmaf(gc.z, gv, sz);
        }
    }
    s0 += __shfl_xor(s0, 16, 64); sx += __shfl_xor(sx, 16, 64); sy += __shfl_xor(sy, 16, 64); sz += __shfl_xor(sz, 16, 64);
    s0 += __shfl_xor(s0, 32, 64); sx += __shfl_xor(sx, 32, 64); sy += __shfl_xor(sy, 32, 64); sz += __shfl_xor(sz, 32, 64);
    gx = fmaf(2.f * px, s0, sx); gy = fmaf(2.f * py, s0, sy); gz = fmaf(2.f * pz, s0, sz);
}

// acc[ct][to] += W relu(x[ct]) for the image at wl (LDS).  k-tile outermost: relu once per operand register, 8 * kSdColTiles
// independent accumulator chains between two uses of the same one (CT column tiles per wave).  kRelu = false: W x[ct], the operand as it is (the
// transposed products of sm_shape_dec_grad.h)
template <bool kRelu = true, int CT>
SM_DEV void sd_linear(const float *wl, int lane, const f32x4 (&x)[CT][8], f32x4 (&acc)[CT][8]) {
#pragma unroll
    for (int ti = 0; ti < 8; ++ti) {
        f32x4 xr[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) xr[ct][r] = kRelu ? fmaxf(x[ct][ti][r], 0.f) : x[ct][ti][r];
#pragma unroll
        for (int to = 0; to < 8; ++to) {
            const float4 a = *reinterpret_cast<const float4 *>(wl + ((to * 8 + ti) * 64 + lane) * 4);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                acc[ct][to] = mfma16(a.x, xr[ct][0], acc[ct][to]);
                acc[ct][to] = mfma16(a.y, xr[ct][1], acc[ct][to]);
                acc[ct][to] = mfma16(a.z, xr[ct][2], acc[ct][to]);
                acc[ct][to] = mfma16(a.w, xr[ct][3], acc[ct][to]);
            }
        }
    }
}

// y[ct][t] = b[16 t + 4 g + r]  (b in LDS)
template <int CT>
SM_DEV void sd_bias(const float *b, int g, f32x4 (&y)[CT][8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const float4 v = *reinterpret_cast<const float4 *>(b + 16 * t + 4 * g);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) y[ct][t] = f32x4{v.x, v.y, v.z, v.w};
    }
}

// x[ct][to] += b + W relu(y[ct]): the block's second Linear.  dx is summed on its own and added to x once, as the reference
// does (a chain started from x would round each of its 128 steps at the magnitude of x); four row tiles at a time, so that
// the dx accumulators cost 16 * CT registers.
template <int CT>
SM_DEV void sd_linear_residual(const float *wl, const float *b, int lane, int g, const f32x4 (&y)[CT][8], f32x4 (&x)[CT][8]) {
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        f32x4 dx[CT][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float4 v = *reinterpret_cast<const float4 *>(b + 16 * (4 * part + t) + 4 * g);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) dx[ct][t] = f32x4{v.x, v.y, v.z, v.w};
        }
#pragma unroll
        for (int ti = 0; ti < 8; ++ti) {
            f32x4 yr[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) yr[ct][r] = fmaxf(y[ct][ti][r], 0.f);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 a = *reinterpret_cast<const float4 *>(wl + (((4 * part + t) * 8 + ti) * 64 + lane) * 4);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    dx[ct][t] = mfma16(a.x, yr[ct][0], dx[ct][t]);
                    dx[ct][t] = mfma16(a.y, yr[ct][1], dx[ct][t]);
                    dx[ct][t] = mfma16(a.z, yr[ct][2], dx[ct][t]);
                    dx[ct][t] = mfma16(a.w, yr[ct][3], dx[ct][t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) x[ct][4 * part + t] += dx[ct][t];
    }
}

// The barrier between two images.  An LDS-DMA piece has landed once the wave that issued it has seen vmcnt reach 0, and is
// visible to the other waves after a barrier that follows: so every wave drains its own pieces here, explicitly, before the
// barrier.  (hipcc also waits before a wave's first LDS read after its own DMA; nothing here relies on that.)
SM_DEV void sd_image_barrier() {
    __builtin_amdgcn_s_waitcnt(0);                         // vmcnt(0) expcnt(0) lgkmcnt(0)
    __syncthreads();
}

__global__ void __launch_bounds__(kSdWaves * 64) sd_decode_kernel(SdArgs a) {
    extern __shared__ float wl[];                          // [2][kSdImg]: the image in use and the next one; [2 L][H] biases
    float *bl = wl + 2 * kSdImg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int64_t n_tiles = (a.n + kSdTile - 1) / kSdTile;
    const int n_lin = 2 * a.L;                             // even: image i always lands in buffer i & 1
    if ((int64_t)blockIdx.x < n_tiles) dma_to_lds(wl, a.img, kSdImg / 4, wave, kSdWaves, lane);
    for (int e = threadIdx.x; e < n_lin * kSdH; e += kSdWaves * 64) bl[e] = a.bias[e];     // visible after the first barrier
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const bool last_tile = tile + gridDim.x >= n_tiles;
        f32x4 x[kSdColTiles][8], y[kSdColTiles][8];
        int64_t pt[kSdColTiles];
        // fc_in: rows 16 t + 4 g + r of this lane's columns
#pragma unroll
        for (int ct = 0; ct < kSdColTiles; ++ct) {
            pt[ct] = tile * kSdTile + (wave * kSdColTiles + ct) * 16 + n;
            float px, py, pz;
            sd_fc_in(a, sd_point(a, pt[ct], px, py, pz), g, px, py, pz, x[ct]);
        }
        for (int i = 0; i < n_lin; i += 2) {
            sd_image_barrier();                            // image i has landed; every wave has left buffer 1 (image i - 1)
            dma_to_lds(wl + kSdImg, a.img + (size_t)(i + 1) * kSdImg, kSdImg / 4, wave, kSdWaves, lane);
            sd_bias(bl + i * kSdH, g, y);                  // net = fc_0(relu(x)) + b0
            sd_linear(wl, lane, x, y);
            sd_image_barrier();                            // image i + 1 has landed; every wave has left buffer 0
            if (i + 2 < n_lin || !last_tile)
                dma_to_lds(wl, a.img + (size_t)(i + 2 < n_lin ? i + 2 : 0) * kSdImg, kSdImg / 4, wave, kSdWaves, lane);
            sd_linear_residual(wl + kSdImg, bl + (i + 1) * kSdH, lane, g, y, x);      // x = x + (fc_1(relu(net)) + b1)
        }
        // fc_out(relu(x)): this lane's 32 rows, then the four lane groups of a column
#pragma unroll
        for (int ct = 0; ct < kSdColTiles; ++ct) {
            const float s = sd_fc_out(a, g, x[ct]);
            if (g == 0 && pt[ct] < a.n) a.out[pt[ct]] = s;
        }
    }
}

// ---- the context's weight block from one flat vector (the one definition of the image layout) ---------------------------------
// Behind the 2 L forward images, for the reverse sweep of sm_shape_dec_grad.h, those of the transposes in reverse order: image
// 2 L + k is W^T of image 2 L - 1 - k.  shapemol_sd_create and shapemol_field_load_weights both launch this kernel.
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
