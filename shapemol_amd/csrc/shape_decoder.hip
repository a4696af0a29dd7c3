// C ABI of the device shape decoder (include/shapemol_hip.h, shapemol_sd_*): DecoderInner.forward of the reference
// (models/shape_pointcloud_modelAE.py:21-103), its gradient with respect to the query points and the gradient shape guidance
// built on it, and the training step (weight and latent gradients, weights from device memory).  Kernels: sm_shape_dec.h,
// sm_shape_dec_grad.h, sm_shape_dec_train.h.
#include "../../include/shapemol_hip.h"
#include "sm_shape_dec_train.h"
#include "sm_devmem.h"
#include "sm_host.h"

#include <hip/hip_ext.h>

#include <atomic>
#include <cmath>
#include <string>
#include <vector>

struct shapemol_sd_ctx;
extern "C" int shapemol_sd_chain_guide_(shapemol_sd_ctx *c, float *pos, const int *mol_of, const int *mol_off, int64_t n_atoms, int64_t n_shapes,
                                        double grad_lr, const int *step_cur, int t_first, int grad_step, hipStream_t s, hipEvent_t e0, hipEvent_t e1);

namespace {
constexpr int kMaxLatent = 256, kMaxLayers = 8, kMaxShapes = 65535;
}  // namespace

struct shapemol_sd_ctx {
    int Z = 32, L = 4, sigmoid = 0, device = 0, n_cu = 1;
    size_t lds_bytes = 0;
    // device memory: every group of buffers beside the capacity it shares (sm_devmem.h: grown by grow(), freed with the context)
    float *d_w = nullptr; DevList mem_w;
    size_t o_zin = 0, o_win = 0, o_bin = 0, o_w0 = 0, o_img = 0, o_bias = 0, o_out = 0;
    // per-shape workspace of the prologue: rewritten by every decode, so a context serves one stream at a time
    int64_t capB = 0, lastB = 0;
    float *zinv = nullptr, *gc = nullptr; DevList mem_B;
    // Identity of this context's device memory (weights and the block above), from a process-wide counter: new at create and
    // at every reallocation of the block, never used twice.  A captured chain step holds d_w and gc and is keyed on it; the
    // context's host address would not do, since a context created after another was destroyed often gets the same address
    uint64_t ws_gen = 0;
    // shapemol_field_guide: the batch vector as int32 [capN] and the molecules' first atoms [capM + 1]
    int64_t capN = 0, capM = 0;
    int *shape_of = nullptr, *mol_off = nullptr; DevList mem_N, mem_M;
    // shapemol_field_train: the chunk workspace (slots, up: capT points; partials of capSplits splits), the float64 accumulators
    // of the blocks' gradients, and per shape (capS) the fc_in sums and dz_inv.  Grown like the per-shape workspace (grow):
    // behind a device synchronise, one stream at a time
    size_t n_weights = 0;
    int64_t capT = 0, capSplits = 0, capS = 0;
    float *tr_slots = nullptr, *tr_up = nullptr, *tr_pw = nullptr, *tr_dzinv = nullptr;
    double *tr_pb = nullptr, *tr_accW = nullptr, *tr_accS = nullptr;
    DevList mem_T, mem_splits, mem_S, mem_accW;
};

namespace {
uint64_t sd_next_identity() {
    static std::atomic<uint64_t> counter{0};
    return ++counter;
}

// the per-shape workspace for n_shapes, then the prologue of z on stream s
int sd_prologue(shapemol_sd_ctx *c, const float *d_z, int64_t n_shapes, hipStream_t s) {
    if (n_shapes > c->capB) c->ws_gen = sd_next_identity();                    // a captured chain step holds gc
    SMCHK(grow(c->mem_B, {dev_buf(&c->zinv, (size_t)n_shapes * c->Z * 4), dev_buf(&c->gc, (size_t)n_shapes * kSdH * 4 * 4)}, c->capB, n_shapes));
    c->lastB = n_shapes;
    const float *W = c->d_w;
    hipLaunchKernelGGL(sd_prologue_kernel, dim3((unsigned)n_shapes), dim3(256), 0, s, d_z, W + c->o_zin, W + c->o_win, W + c->o_bin, c->Z, c->zinv, c->gc);
    return 0;
}

// the offsets of the context's block, every piece on a 64-float boundary; returns the block's floats
size_t sd_layout(shapemol_sd_ctx *c) {
    size_t end = 0;
    auto put = [&](size_t n) { const size_t o = (end + 63) & ~size_t(63); end = o + n; return o; };
    const size_t H = kSdH, Z = c->Z, L = c->L;
    c->o_zin = put(Z * Z); c->o_win = put(H * (2 * Z + 1)); c->o_bin = put(H); c->o_w0 = put(H);
    c->o_img = put(4 * L * kSdImg); c->o_bias = put(2 * L * H); c->o_out = put(H + 1);
    return end;
}

// the block's contents from a flat device vector in the weights' order (sd_repack_kernel, sm_shape_dec.h)
void sd_repack(const shapemol_sd_ctx *c, const float *d_weights, hipStream_t s) {
    SdRepackArgs a{};
    a.w = d_weights; a.dst = c->d_w; a.o_zin = c->o_zin; a.o_win = c->o_win; a.o_bin = c->o_bin; a.o_w0 = c->o_w0; a.o_img = c->o_img;
    a.o_bias = c->o_bias; a.o_out = c->o_out; a.Z = c->Z; a.L = c->L;
    hipLaunchKernelGGL(sd_repack_kernel, dim3(16, 1 + 2 * c->L), dim3(256), 0, s, a);
}

SdArgs sd_args(const shapemol_sd_ctx *c, const float *d_p, const int32_t *d_shape_of, int64_t n_points, int64_t points_per_shape, int64_t n_shapes, float *d_out) {
    const float *W = c->d_w;
    SdArgs a{};
    a.p = d_p; a.shape_of = d_shape_of; a.gc = c->gc; a.w0 = W + c->o_w0; a.img = W + c->o_img; a.bias = W + c->o_bias; a.w_out = W + c->o_out;
    a.out = d_out; a.n = n_points; a.per_shape = points_per_shape > 0 ? points_per_shape : 1; a.B = (int)n_shapes; a.L = c->L; a.sigmoid = c->sigmoid;
    return a;
}
// one workgroup per CU (its two weight images fill most of the CU's LDS), striding over the tiles
unsigned sd_grid(const shapemol_sd_ctx *c, int64_t n_points, int tile = kSdTile) {
    const int64_t n_tiles = (n_points + tile - 1) / tile;
    return (unsigned)(n_tiles < c->n_cu ? n_tiles : c->n_cu);
}

// the argument checks that shapemol_sd_decode and shapemol_field_decode_grad share
int sd_check(const std::string &me, const shapemol_sd_ctx *c, int64_t n_points, int64_t points_per_shape, bool has_shape_of, int64_t n_shapes) {
    if (!c) return sm_fail(me + ": null context");
    if (n_shapes < 1 || n_shapes > kMaxShapes) return sm_fail(me + ": n_shapes must be in 1..65535, got " + std::to_string(n_shapes));
    if (n_points < 0 || n_points >= ((int64_t)1 << 31))
        return sm_fail(me + ": n_points must be below 2^31 = 2147483648, got " + std::to_string(n_points));
    if (!has_shape_of && (points_per_shape < 0 || n_points != n_shapes * points_per_shape))
        return sm_fail(me + ": without shape_of, n_points must be n_shapes * points_per_shape; got " + std::to_string(n_points) +
                       " points for " + std::to_string(n_shapes) + " x " + std::to_string(points_per_shape));
    return 0;
}
}  // namespace

extern "C" {

size_t shapemol_sd_weight_count(int32_t hidden, int32_t latent, int32_t layer_num) {
    const size_t H = hidden, Z = latent, L = layer_num;
    return Z * Z + H * (2 * Z + 1) + H + L * (2 * H * H + 2 * H) + H + 1;
}

int shapemol_sd_create(int32_t hidden, int32_t latent, int32_t layer_num, int32_t loss_type, const float *w, size_t n_weights,
                       int device, shapemol_sd_ctx **out) {
    if (!w || !out) return sm_fail("shapemol_sd_create: null argument");
    if (hidden != kSdH) return sm_fail("shapemol_sd_create: hidden must be 128, got " + std::to_string(hidden));
    if (latent < 1 || latent > kMaxLatent) return sm_fail("shapemol_sd_create: latent must be in 1..256, got " + std::to_string(latent));
    if (layer_num < 1 || layer_num > kMaxLayers) return sm_fail("shapemol_sd_create: layer_num must be in 1..8, got " + std::to_string(layer_num));
    if (loss_type != SHAPEMOL_SD_SIGNEDDIST && loss_type != SHAPEMOL_SD_OCCUPANCY)
        return sm_fail("shapemol_sd_create: loss_type must be SHAPEMOL_SD_SIGNEDDIST (0) or SHAPEMOL_SD_OCCUPANCY (1), got " + std::to_string(loss_type));
    const size_t need = shapemol_sd_weight_count(hidden, latent, layer_num);
    if (n_weights != need)
        return sm_fail("shapemol_sd_create: weight count mismatch: " + std::to_string(n_weights) + " given, " + std::to_string(need) + " needed");
    if (sm_open_device(device, "shapemol_sd_create")) return 1;
    int lds = 0, n_cu = 0;
    SMCHK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    SMCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    const int H = kSdH, Z = latent, L = layer_num;
    const size_t lds_bytes = ((size_t)2 * kSdImg + (size_t)2 * L * H) * sizeof(float);
    if ((size_t)lds < lds_bytes)
        return sm_fail("shapemol_sd_create: the decode kernel needs " + std::to_string(lds_bytes) + " bytes of LDS per workgroup, the device has " + std::to_string(lds));
    // once per context, not per decode; the largest image set (layer_num 8) where it fits, so that contexts of different
    // depths do not shrink each other's limit
    const int lds_all = (int)(((size_t)2 * kSdImg + (size_t)2 * kMaxLayers * H) * sizeof(float));
    SMCHK(hipFuncSetAttribute((const void *)sd_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_all <= lds ? lds_all : (int)lds_bytes));
    SMCHK(hipFuncSetAttribute((const void *)sd_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_all <= lds ? lds_all : (int)lds_bytes));
    SMCHK(hipFuncSetAttribute((const void *)sd_train_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_all <= lds ? lds_all : (int)lds_bytes));
    auto *c = new shapemol_sd_ctx();
    c->ws_gen = sd_next_identity();
    c->n_weights = need;
    c->Z = Z; c->L = L; c->sigmoid = loss_type == SHAPEMOL_SD_OCCUPANCY; c->device = device; c->n_cu = n_cu > 0 ? n_cu : 1; c->lds_bytes = lds_bytes;
    // the block, then its contents by the kernel that holds the layout (sd_repack_kernel), from a staging copy of w
    const size_t n_block = sd_layout(c);
    float *stage = nullptr;
    DevList mem_stage;                                                          // (freed when this function returns)
    hipError_t e = c->mem_w.alloc(&c->d_w, n_block * 4, true);                  // (zeroed: the alignment gaps)
    if (e == hipSuccess) e = mem_stage.alloc(&stage, need * 4);
    if (e == hipSuccess) e = hipMemcpy(stage, w, need * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) { sd_repack(c, stage, nullptr); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        delete c; return sm_fail(std::string("shapemol_sd_create: device allocation failed: ") + hipGetErrorString(e));
    }
    *out = c;
    return 0;
}

void shapemol_sd_destroy(shapemol_sd_ctx *c) {
    if (!c) return;
    sm_close_device(c->device);
    delete c;                // its lists release what they own
}

int64_t shapemol_sd_tile(const shapemol_sd_ctx *c) { return c ? kSdTile : 0; }
int64_t shapemol_field_grad_tile(const shapemol_sd_ctx *c) { return c ? kSdGradTile : 0; }

int shapemol_sd_decode(shapemol_sd_ctx *c, const float *d_p, const int32_t *d_shape_of, int64_t n_points, int64_t points_per_shape,
                       const float *d_z, int64_t n_shapes, float *d_out, void *stream) {
    if (sd_check("shapemol_sd_decode", c, n_points, points_per_shape, d_shape_of != nullptr, n_shapes)) return 1;
    if (n_points == 0) return 0;
    if (!d_p || !d_z || !d_out) return sm_fail("shapemol_sd_decode: null argument");
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (sd_prologue(c, d_z, n_shapes, s)) return 1;
    const SdArgs a = sd_args(c, d_p, d_shape_of, n_points, points_per_shape, n_shapes, d_out);
    hipLaunchKernelGGL(sd_decode_kernel, dim3(sd_grid(c, n_points)), dim3(kSdWaves * 64), c->lds_bytes, s, a);
    SMCHK(hipGetLastError());
    return 0;
}

int shapemol_field_decode_grad(shapemol_sd_ctx *c, const float *d_p, const int32_t *d_shape_of, int64_t n_points, int64_t points_per_shape,
                            const float *d_z, int64_t n_shapes, float *d_out, float *d_grad, void *stream) {
    if (sd_check("shapemol_field_decode_grad", c, n_points, points_per_shape, d_shape_of != nullptr, n_shapes)) return 1;
    if (n_points == 0) return 0;
    if (!d_p || !d_z || !d_grad) return sm_fail("shapemol_field_decode_grad: null argument");
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (sd_prologue(c, d_z, n_shapes, s)) return 1;
    SdGradArgs ga{};
    ga.d = sd_args(c, d_p, d_shape_of, n_points, points_per_shape, n_shapes, d_out);
    ga.grad = d_grad;
    hipLaunchKernelGGL(sd_grad_kernel, dim3(sd_grid(c, n_points, kSdGradTile)), dim3(kSdGradWaves * 64), c->lds_bytes, s, ga);
    SMCHK(hipGetLastError());
    return 0;
}

int shapemol_field_guide(shapemol_sd_ctx *c, float *d_pos, const int64_t *d_batch, int64_t n_atoms, const float *d_z, int64_t n_shapes,
                      double grad_lr, void *stream) {
    if (!c) return sm_fail("shapemol_field_guide: null context");
    if (n_shapes < 1 || n_shapes > kMaxShapes) return sm_fail("shapemol_field_guide: n_shapes must be in 1..65535, got " + std::to_string(n_shapes));
    if (n_atoms < 0 || n_atoms > (1 << 27)) return sm_fail("shapemol_field_guide: n_atoms must be at most 2^27 = 134217728, got " + std::to_string(n_atoms));
    if (!std::isfinite(grad_lr)) return sm_fail("shapemol_field_guide: grad_lr is not finite");
    if (n_atoms == 0) return 0;
    if (!d_pos || !d_batch || !d_z) return sm_fail("shapemol_field_guide: null argument");
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    SMCHK(grow(c->mem_N, {dev_buf(&c->shape_of, (size_t)n_atoms * 4)}, c->capN, n_atoms));
    SMCHK(grow(c->mem_M, {dev_buf(&c->mol_off, (size_t)(n_shapes + 1) * 4)}, c->capM, n_shapes));
    if (sd_prologue(c, d_z, n_shapes, s)) return 1;
    const int64_t work = n_atoms > n_shapes + 1 ? n_atoms : n_shapes + 1;
    hipLaunchKernelGGL(sd_batch_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, d_batch, (int)n_atoms, (int)n_shapes, c->shape_of, c->mol_off);
    return shapemol_sd_chain_guide_(c, d_pos, c->shape_of, c->mol_off, n_atoms, n_shapes, grad_lr, nullptr, 0, 0, s, nullptr, nullptr);
}

// ---- training (sm_shape_dec_train.h) -----------------------------------------------------------------------------------------
int64_t shapemol_field_train_tile(const shapemol_sd_ctx *c) { return c ? kSdTrainTile : 0; }

int shapemol_field_load_weights(shapemol_sd_ctx *c, const float *d_weights, size_t n_weights, void *stream) {
    if (!c) return sm_fail("shapemol_field_load_weights: null context");
    if (!d_weights) return sm_fail("shapemol_field_load_weights: null argument");
    if (n_weights != c->n_weights)
        return sm_fail("shapemol_field_load_weights: weight count mismatch: " + std::to_string(n_weights) + " given, " + std::to_string(c->n_weights) + " needed");
    SMCHK(hipSetDevice(c->device));
    sd_repack(c, d_weights, (hipStream_t)stream);
    SMCHK(hipGetLastError());
    c->ws_gen = sd_next_identity();                        // a captured chain step was recorded with the old field: it is captured again
    return 0;
}

int shapemol_field_train(shapemol_sd_ctx *c, const float *d_p, int64_t n_shapes, int64_t points_per_shape, const float *d_z, const float *d_upstream,
                         float *d_out, float *d_grad_p, float *d_grad_z, float *d_grad_weights, int64_t chunk_points, void *stream) {
    const std::string me = "shapemol_field_train";
    if (!c) return sm_fail(me + ": null context");
    if (points_per_shape < 0 || points_per_shape >= ((int64_t)1 << 31)) return sm_fail(me + ": points_per_shape must be in 0 .. 2^31 - 1, got " + std::to_string(points_per_shape));
    const int64_t n_points = n_shapes * points_per_shape;
    if (sd_check(me, c, n_points, points_per_shape, false, n_shapes)) return 1;
    if (chunk_points < 0 || chunk_points % kSdTrainTile)
        return sm_fail(me + ": chunk_points must be 0 (the default) or a multiple of the tile (" + std::to_string(kSdTrainTile) + "), got " + std::to_string(chunk_points));
    if (!d_upstream) return sm_fail(me + ": null upstream gradient");
    if (!d_z || !d_grad_z || !d_grad_weights || (n_points > 0 && !d_p)) return sm_fail(me + ": null argument");
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int L = c->L, Z = c->Z;
    if (n_points == 0) {
        SMCHK(hipMemsetAsync(d_grad_z, 0, (size_t)n_shapes * Z * 3 * 4, s));
        SMCHK(hipMemsetAsync(d_grad_weights, 0, c->n_weights * 4, s));
        return 0;
    }
    const int64_t all_tiles = (n_points + kSdTrainTile - 1) / kSdTrainTile;
    int64_t chunk = chunk_points ? chunk_points : (int64_t)c->n_cu * kSdTrainTile;
    if (chunk > all_tiles * kSdTrainTile) chunk = all_tiles * kSdTrainTile;
    auto splits_of = [](int64_t groups) { const int64_t v = (groups + 7) / 8; return (int)(v < kSdMaxSplits ? v : kSdMaxSplits); };
    const int need_splits = splits_of(chunk / 16);
    SMCHK(grow(c->mem_T, {dev_buf(&c->tr_slots, (size_t)(4 * L + 2) * chunk * kSdH * 4), dev_buf(&c->tr_up, (size_t)chunk * 4)}, c->capT, chunk));
    SMCHK(grow(c->mem_splits, {dev_buf(&c->tr_pw, (size_t)2 * L * need_splits * kSdImg * 4), dev_buf(&c->tr_pb, (size_t)2 * L * need_splits * kSdH * 8)},
               c->capSplits, need_splits));
    SMCHK(grow(c->mem_S, {dev_buf(&c->tr_accS, (size_t)n_shapes * kSdSums * kSdH * 8), dev_buf(&c->tr_dzinv, (size_t)n_shapes * Z * 4)}, c->capS, n_shapes));
    if (!c->tr_accW) SMCHK(c->mem_accW.alloc(&c->tr_accW, (size_t)2 * L * (kSdImg + kSdH) * 8));    // once: its size is the context's
    if (sd_prologue(c, d_z, n_shapes, s)) return 1;
    const size_t slot_sz = (size_t)c->capT * kSdH;
    const int lin_blocks = (kSdImg + kSdH + 255) / 256;
    for (int64_t first = 0; first < n_points; first += chunk) {
        const int64_t n = n_points - first < chunk ? n_points - first : chunk;
        const int64_t groups = (n + kSdTrainTile - 1) / kSdTrainTile * (kSdTrainTile / 16);
        SdTrainArgs ta{};
        ta.d = sd_args(c, d_p + first * 3, nullptr, n, points_per_shape, n_shapes, d_out ? d_out + first : nullptr);
        ta.first = first; ta.up_in = d_upstream + first; ta.grad = d_grad_p ? d_grad_p + first * 3 : nullptr;
        ta.slots = c->tr_slots; ta.up = c->tr_up; ta.cap = c->capT;
        hipLaunchKernelGGL(sd_train_kernel, dim3(sd_grid(c, n, kSdTrainTile)), dim3(kSdGradWaves * 64), c->lds_bytes, s, ta);
        int splits = splits_of(groups);
        const int per_split = (int)((groups + splits - 1) / splits);
        splits = (int)((groups + per_split - 1) / per_split);
        hipLaunchKernelGGL(sd_dw_kernel, dim3(2 * L, splits), dim3(256), 0, s, c->tr_slots, slot_sz, L, groups, per_split, c->tr_pw, c->tr_pb);
        hipLaunchKernelGGL(sd_dw_reduce_kernel, dim3(lin_blocks, 2 * L), dim3(256), 0, s, c->tr_pw, c->tr_pb, splits, first == 0 ? 1 : 0, c->tr_accW);
        hipLaunchKernelGGL(sd_shape_sums_kernel, dim3((unsigned)n_shapes), dim3(512), 0, s, c->tr_slots, slot_sz, L, c->tr_up, d_p + first * 3, first, n,
                           points_per_shape, first == 0 ? 1 : 0, c->tr_accS);
    }
    const float *W = c->d_w;
    hipLaunchKernelGGL(sd_prologue_back_kernel, dim3((unsigned)n_shapes), dim3(256), 0, s, d_z, W + c->o_zin, W + c->o_win, Z, c->tr_accS, c->tr_dzinv, d_grad_z);
    const size_t n_head = (size_t)Z * Z + (size_t)kSdH * (2 * Z + 1) + kSdH, o_out = n_head + (size_t)2 * L * (kSdImg + kSdH);
    hipLaunchKernelGGL(sd_head_weights_kernel, dim3((unsigned)((n_head + kSdH + 1 + 255) / 256)), dim3(256), 0, s, d_z, c->zinv, c->tr_dzinv, c->tr_accS, Z,
                       (int)n_shapes, o_out, d_grad_weights);
    hipLaunchKernelGGL(sd_dw_finish_kernel, dim3(lin_blocks, 2 * L), dim3(256), 0, s, c->tr_accW, d_grad_weights + n_head);
    SMCHK(hipGetLastError());
    return 0;
}

// ---- for shapemol_hip.hip (field guidance inside a chain; not in the header) -----------------------------------------------
void shapemol_sd_describe_(const shapemol_sd_ctx *c, int *device, int *latent) { *device = c->device; *latent = c->Z; }

// the chain's prep: the prologue of the chain's shapes; *gen = the identity of the device memory a captured step would hold
int shapemol_sd_chain_prepare_(shapemol_sd_ctx *c, const float *d_z, int64_t n_shapes, hipStream_t s, uint64_t *gen) {
    if (n_shapes < 1 || n_shapes > kMaxShapes) return sm_fail("field guidance: the decoder takes 1..65535 shapes, the chain has " + std::to_string(n_shapes));
    if (sd_prologue(c, d_z, n_shapes, s)) return 1;
    *gen = c->ws_gen;
    SMCHK(hipGetLastError());
    return 0;
}

// one guidance pass on pos with the prologue's data as it stands (mol_of sorted in [0, B), mol_off [B + 1]); with events, a
// profiled launch
int shapemol_sd_chain_guide_(shapemol_sd_ctx *c, float *pos, const int *mol_of, const int *mol_off, int64_t n_atoms, int64_t n_shapes, double grad_lr,
                             const int *step_cur, int t_first, int grad_step, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    SdGradArgs ga{};
    ga.d = sd_args(c, pos, mol_of, n_atoms, 0, n_shapes, nullptr);
    ga.pos = pos; ga.mol_off = mol_off; ga.lr = (float)grad_lr; ga.step_cur = step_cur; ga.t_first = t_first; ga.grad_step = grad_step;
    const dim3 grid(sd_grid(c, n_atoms, kSdGradTile)), block(kSdGradWaves * 64);
    if (e0) hipExtLaunchKernelGGL(sd_grad_kernel, grid, block, c->lds_bytes, s, e0, e1, 0, ga);
    else hipLaunchKernelGGL(sd_grad_kernel, grid, block, c->lds_bytes, s, ga);
    SMCHK(hipGetLastError());
    return 0;
}

int shapemol_sd_debug_read(shapemol_sd_ctx *c, int32_t what, void *h_dst, size_t n_bytes) {
    if (!c || !h_dst) return sm_fail("shapemol_sd_debug_read: null argument");
    if (c->lastB == 0) return sm_fail("shapemol_sd_debug_read: no shapemol_sd_decode has run on this context");
    const size_t B = (size_t)c->lastB, H = kSdH, Z = c->Z;
    if (what < SHAPEMOL_SD_ZINV || what > SHAPEMOL_SD_C)
        return sm_fail("shapemol_sd_debug_read: what must be SHAPEMOL_SD_ZINV, SHAPEMOL_SD_G or SHAPEMOL_SD_C (0 .. 2), got " + std::to_string(what));
    const size_t need = what == SHAPEMOL_SD_ZINV ? B * Z * 4 : what == SHAPEMOL_SD_G ? B * H * 3 * 4 : B * H * 4;
    if (n_bytes != need) return sm_fail("shapemol_sd_debug_read: buffer " + std::to_string(what) + " of the last decode has " + std::to_string(need) + " bytes, n_bytes is " + std::to_string(n_bytes));
    SMCHK(hipSetDevice(c->device));
    SMCHK(hipDeviceSynchronize());
    if (what == SHAPEMOL_SD_ZINV) { SMCHK(hipMemcpy(h_dst, c->zinv, need, hipMemcpyDeviceToHost)); return 0; }
    std::vector<float> gc(B * H * 4);
    SMCHK(hipMemcpy(gc.data(), c->gc, gc.size() * 4, hipMemcpyDeviceToHost));
    float *dst = (float *)h_dst;
    for (size_t e = 0; e < B * H; ++e) {
        if (what == SHAPEMOL_SD_G) for (int k = 0; k < 3; ++k) dst[e * 3 + k] = gc[e * 4 + k];
        else dst[e] = gc[e * 4 + 3];
    }
    return 0;
}

}  // extern "C"
