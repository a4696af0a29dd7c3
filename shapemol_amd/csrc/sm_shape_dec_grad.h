// The shape decoder's value AND its gradient with respect to the query point in one pass (reverse mode), and behind it the
// reference's gradient shape guidance (models/molopt_score_model.py:592-615, the `use_grad` branch of sample_diffusion).
//
// Forward: sd_decode_kernel's arithmetic, call for call (sd_fc_in, sd_linear, sd_linear_residual, sd_fc_out), so the value is
// the decode kernel's bit for bit.  While going forward the kernel keeps one bit per ReLU input, m = (v > 0) (torch's
// convention at 0): 2 L + 1 inputs of 128 units.  A lane holds rows 16 t + 4 g + r of its columns, so its 32 bits of an input
// are ONE dword per column tile, bit 4 t + r -- and since a Linear's output layout is the next one's operand layout, the bits
// a lane keeps are those of the rows it holds, forward and backward.
//
// Backward, in the same layout, on the same fp32-input matrix cores:
//     g   = w_out (.) m_last                          (times s (1 - s) for occupancy)
//     for every block, last to first:   g_y = m_y (.) (W1^T g),    g = g + m_x (.) (W0^T g_y)
//     grad = 2 p (w0 . g) + G_b^T g
// The transposed images (same wimg layout, of W^T) lie behind the forward ones in the order the backward pass wants them:
// image 2 L + k is the transpose of image 2 L - 1 - k.  So the 4 L images of a tile stream through the decode kernel's
// two-buffer pipeline unchanged: image j lands in buffer j & 1, one sd_image_barrier per image.
//
// Guidance epilogue (a.pos != null): with d the value, T_j the atom count of the point's molecule (= its shape),
//     p <- p - grad_lr (min(d, 0.5) - 0.5) (1[d < 0.5] / T_j) grad
// in place.  In a chain the launch is part of the captured step and reads the device step counter for `t > grad_step`.
#pragma once
#include "sm_shape_dec.h"

constexpr int kSdMaxL = 8;                                 // layer_num limit of shapemol_sd_create
// The masks cost 2 L + 1 registers per column tile on top of the decode kernel's 250, and its eight waves have 256 each.  So
// FOUR waves of two column tiles: one wave per SIMD, which may use the whole register file (VGPR + AGPR); a tile of 128 points
// (every edge of the decode kernel's tile of 256 is one of this tile's too).  Four waves of four column tiles want about 420
// registers and hipcc then spills to scratch memory.
constexpr int kSdGradWaves = 4, kSdGradColTiles = 2;
constexpr int kSdGradTile = kSdGradWaves * kSdGradColTiles * 16;
constexpr int kSdMasks = 2 * kSdMaxL + 1;

struct SdGradArgs {
    SdArgs d;                // the forward's arguments; d.img: 4 L images (above); d.out may be null
    float *grad;             // [n][3] or null
    float *pos;              // guidance: [n][3], == d.p, updated in place; else null
    const int *mol_off;      // guidance: [B + 1] first atom of every molecule (d.shape_of is the sorted molecule index)
    float lr;                // guidance: grad_lr
    const int *step_cur;     // chain: the device's reverse-step counter, else null (always applied)
    int t_first, grad_step;  // chain: step s is guided when t_first - s > grad_step

    // sd_sweep's Mode (below)
    static constexpr bool kTaps = false;
    SM_DEV int64_t point(int64_t pt, float &px, float &py, float &pz) const { return sd_point(d, pt, px, py, pz); }
    SM_DEV float top(int, int64_t, float val) const { return d.sigmoid ? val * (1.f - val) : 1.f; }
    SM_DEV void epilogue(int64_t q, int64_t sb, float val, float px, float py, float pz, float gx, float gy, float gz) const {
        if (pos && val < 0.5f) {                           // the guidance update
            const int cnt = mol_off[sb + 1] - mol_off[sb];
            const float k = lr * (val - 0.5f), inv = 1.f / (float)(cnt > 0 ? cnt : 1);
            pos[q * 3] = px - k * (inv * gx); pos[q * 3 + 1] = py - k * (inv * gy); pos[q * 3 + 2] = pz - k * (inv * gz);
        }
    }
};

// bit 4 t + r = (x[t][r] > 0)
SM_DEV unsigned sd_relu_mask(const f32x4 (&x)[8]) {
    unsigned m = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) m |= (x[t][r] > 0.f ? 1u : 0u) << (4 * t + r);
    return m;
}
// The masks live in registers; `idx` is uniform but not a constant, so a slot is picked with a chain of selects (a register
// array indexed by a variable would go to scratch memory)
SM_DEV void sd_mask_put(unsigned (&mk)[kSdMasks], int idx, unsigned m) {
#pragma unroll
    for (int k = 0; k < kSdMasks; ++k) mk[k] = k == idx ? m : mk[k];
}
SM_DEV unsigned sd_mask_get(const unsigned (&mk)[kSdMasks], int idx) {
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < kSdMasks; ++k) m = k == idx ? mk[k] : m;
    return m;
}
SM_DEV void sd_mask_apply(unsigned m, f32x4 (&x)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) x[t][r] = (m >> (4 * t + r)) & 1u ? x[t][r] : 0.f;
}

// g[ct] += m[ct] (.) (W gy[ct]) for the image at wl: the block's first Linear backwards.  Four row tiles at a time, like
// sd_linear_residual
SM_DEV void sd_linear_back_residual(const float *wl, int lane, const f32x4 (&gy)[kSdGradColTiles][8], const unsigned (&m)[kSdGradColTiles],
                                    f32x4 (&gx)[kSdGradColTiles][8]) {
    constexpr int RT = 4;
#pragma unroll
    for (int part = 0; part < 8 / RT; ++part) {
        f32x4 dx[kSdGradColTiles][RT];
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int ct = 0; ct < kSdGradColTiles; ++ct) dx[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ti = 0; ti < 8; ++ti) {
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                const float4 a = *reinterpret_cast<const float4 *>(wl + (((RT * part + t) * 8 + ti) * 64 + lane) * 4);
#pragma unroll
                for (int ct = 0; ct < kSdGradColTiles; ++ct) {
                    dx[ct][t] = mfma16(a.x, gy[ct][ti][0], dx[ct][t]);
                    dx[ct][t] = mfma16(a.y, gy[ct][ti][1], dx[ct][t]);
                    dx[ct][t] = mfma16(a.z, gy[ct][ti][2], dx[ct][t]);
                    dx[ct][t] = mfma16(a.w, gy[ct][ti][3], dx[ct][t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int ct = 0; ct < kSdGradColTiles; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if ((m[ct] >> (4 * (RT * part + t) + r)) & 1u) gx[ct][RT * part + t][r] += dx[ct][t][r];
    }
}

// The forward and reverse sweep over a workgroup's tiles: the one body of sd_grad_kernel and of sd_train_kernel
// (sm_shape_dec_train.h).  Mode is the kernel's argument struct; what the two kernels do differently is decided when the body is
// specialised, never at run time:
//     m.point(pt, px, py, pz)      the point and its shape (sd_point's contract)
//     m.top(g, pt, val)            the factor on w_out at the top of the way back
//     Mode::kTaps, m.tap(..)       training: the sweep's operands and upstream gradients go out to slots as they are formed
//     m.grad                       [n][3] or null
//     m.epilogue(..)               after value and gradient are stored
template <class Mode>
SM_DEV void sd_sweep(const SdArgs &a, const Mode &m) {
    extern __shared__ float wl[];                          // [2][kSdImg]: the image in use and the next one; [2 L][H] biases
    float *bl = wl + 2 * kSdImg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int64_t n_tiles = (a.n + kSdGradTile - 1) / kSdGradTile;
    const int n_lin = 2 * a.L, n_img = 4 * a.L;            // even: image j always lands in buffer j & 1
    if ((int64_t)blockIdx.x < n_tiles) dma_to_lds(wl, a.img, kSdImg / 4, wave, kSdGradWaves, lane);
    for (int e = threadIdx.x; e < n_lin * kSdH; e += kSdGradWaves * 64) bl[e] = a.bias[e];     // visible after the first barrier
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
            grp[ct] = tile * (kSdGradTile / 16) + wave * kSdGradColTiles + ct;
            pt[ct] = grp[ct] * 16 + n;
            // (guidance: a tail lane may read the last point while its owner stores the update; a tail's result is dropped)
            sb[ct] = m.point(pt[ct], px[ct], py[ct], pz[ct]);
            sd_fc_in(a, sb[ct], g, px[ct], py[ct], pz[ct], x[ct]);
        }
        // ---- forward: as sd_decode_kernel, keeping the masks of x (slot 2 b) and net (slot 2 b + 1) of block b
        for (int i = 0; i < n_lin; i += 2) {
            sd_image_barrier();                            // image i has landed; every wave has left buffer 1 (image i - 1)
            dma_to_lds(wl + kSdImg, a.img + (size_t)(i + 1) * kSdImg, kSdImg / 4, wave, kSdGradWaves, lane);
#pragma unroll
            for (int ct = 0; ct < kSdGradColTiles; ++ct) {
                sd_mask_put(mk[ct], i, sd_relu_mask(x[ct]));
                if constexpr (Mode::kTaps) m.tap(i, grp[ct], lane, x[ct], true);
            }
            sd_bias(bl + i * kSdH, g, y);
            sd_linear(wl, lane, x, y);
            sd_image_barrier();                            // image i + 1 has landed; every wave has left buffer 0
            dma_to_lds(wl, a.img + (size_t)(i + 2) * kSdImg, kSdImg / 4, wave, kSdGradWaves, lane);      // (i + 2 <= 2 L < 4 L)
#pragma unroll
            for (int ct = 0; ct < kSdGradColTiles; ++ct) {
                sd_mask_put(mk[ct], i + 1, sd_relu_mask(y[ct]));
                if constexpr (Mode::kTaps) m.tap(i + 1, grp[ct], lane, y[ct], true);
            }
            sd_linear_residual(wl + kSdImg, bl + (i + 1) * kSdH, lane, g, y, x);
        }
        // ---- fc_out, and its way back: g = f w_out (.) m_last with f = m.top(..); x becomes g
        float val[kSdGradColTiles];
#pragma unroll
        for (int ct = 0; ct < kSdGradColTiles; ++ct) {
            val[ct] = sd_fc_out(a, g, x[ct]);
            const unsigned mask = sd_relu_mask(x[ct]);
            const float f = m.top(g, pt[ct], val[ct]);
            if constexpr (Mode::kTaps) {                   // slot 4 L + 1 takes f relu(x_L)
#pragma unroll
                for (int t = 0; t < 8; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[ct][t][r] = f * fmaxf(x[ct][t][r], 0.f);
                m.tap(n_img + 1, grp[ct], lane, y[ct], false);
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float4 w = ldg4(a.w_out + 16 * t + 4 * g);
                x[ct][t] = f32x4{w.x * f, w.y * f, w.z * f, w.w * f};
            }
            sd_mask_apply(mask, x[ct]);
        }
        // ---- backward through the blocks: images 2 L + 2 k (W1^T) and 2 L + 2 k + 1 (W0^T) of block L - 1 - k; the taps take
        // dY of fc_1 (g) and of fc_0 (g_y)
        for (int j = n_lin; j < n_img; j += 2) {
            const int b = (n_img - 2 - j) >> 1;
            sd_image_barrier();                            // image j has landed; every wave has left buffer 1
            dma_to_lds(wl + kSdImg, a.img + (size_t)(j + 1) * kSdImg, kSdImg / 4, wave, kSdGradWaves, lane);
#pragma unroll
            for (int ct = 0; ct < kSdGradColTiles; ++ct) {
                if constexpr (Mode::kTaps) m.tap(n_lin + 2 * b + 1, grp[ct], lane, x[ct], false);
#pragma unroll
                for (int t = 0; t < 8; ++t) y[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            sd_linear<false>(wl, lane, x, y);              // g_y = m_y (.) (W1^T g)
            unsigned mx[kSdGradColTiles];
#pragma unroll
            for (int ct = 0; ct < kSdGradColTiles; ++ct) {
                sd_mask_apply(sd_mask_get(mk[ct], 2 * b + 1), y[ct]);
                mx[ct] = sd_mask_get(mk[ct], 2 * b);
                if constexpr (Mode::kTaps) m.tap(n_lin + 2 * b, grp[ct], lane, y[ct], false);
            }
            sd_image_barrier();                            // image j + 1 has landed; every wave has left buffer 0
            if (j + 2 < n_img || !last_tile)
                dma_to_lds(wl, a.img + (size_t)(j + 2 < n_img ? j + 2 : 0) * kSdImg, kSdImg / 4, wave, kSdGradWaves, lane);
            sd_linear_back_residual(wl + kSdImg, lane, y, mx, x);      // g = g + m_x (.) (W0^T g_y)
        }
        // ---- fc_in backwards (the tap takes g at its output), then the stores and the epilogue
#pragma unroll
        for (int ct = 0; ct < kSdGradColTiles; ++ct) {
            if constexpr (Mode::kTaps) m.tap(n_img, grp[ct], lane, x[ct], false);
            float gx, gy, gz;
            sd_fc_in_back(a, sb[ct], g, px[ct], py[ct], pz[ct], x[ct], gx, gy, gz);
            if (g != 0 || pt[ct] >= a.n) continue;
            const int64_t q = pt[ct];
            if (a.out) a.out[q] = val[ct];
            if (m.grad) { m.grad[q * 3] = gx; m.grad[q * 3 + 1] = gy; m.grad[q * 3 + 2] = gz; }
            m.epilogue(q, sb[ct], val[ct], px[ct], py[ct], pz[ct], gx, gy, gz);
        }
    }
}

__global__ void __launch_bounds__(kSdGradWaves * 64) sd_grad_kernel(SdGradArgs ga) {
    if (ga.step_cur && ga.t_first - *ga.step_cur <= ga.grad_step) return;      // `if i > grad_step` (molopt_score_model.py:595)
    sd_sweep(ga.d, ga);
}

// shapemol_field_guide: the batch vector as the kernel wants it -- shape_of [n] = batch (int32), mol_off [B + 1] = first atom of
// every molecule of the SORTED vector (lower bound)
__global__ void __launch_bounds__(256) sd_batch_kernel(const int64_t *batch, int n, int B, int *shape_of, int *mol_off) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int64_t b = batch[i];
        shape_of[i] = (int)(b < 0 ? 0 : (b >= B ? B - 1 : b));
    }
    if (i <= B) {
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (batch[mid] < (int64_t)i) lo = mid + 1; else hi = mid;
        }
        mol_off[i] = lo;
    }
}
