// C ABI of the device shape encoder (include/shapemol_hip.h, shapemol_se_*): VN_DGCNN_Encoder.forward of the reference
// (models/shape_pointcloud_modelAE.py:207-255), its training variant and its backward.  Kernels: sm_shape.h, sm_shape_train.h.
// One forward sweep, se_forward, serves shapemol_se_encode and shapemol_se_train_forward: they differ in where the results go and
// in how the batch sums are taken (SeForwardDst).  One packer, se_pack_weights, a kernel, builds the weight image for
// shapemol_se_create and shapemol_se_load_weights.
#include "../../include/shapemol_hip.h"
#include "sm_shape.h"
#include "sm_shape_train.h"
#include "sm_devmem.h"
#include "sm_host.h"

#include <string>
#include <vector>

namespace {
constexpr int kC = 128;          // hidden_dim of the shipped shape auto-encoder (se_model.pt: config.model.hidden_dim)
}  // namespace

struct shapemol_se_ctx {
    int C = kC, LAT = 32, L = 4, device = 0;
    int lds_limit = 0, max_n = 0;   // largest dynamic LDS of a workgroup on the device; largest N whose 16 x N d2 rows fit in it
    int stop_after = -1;            // shapemol_se_debug_stop_after
    int64_t lastP = 0;              // points of the last encode (shapemol_se_debug_read)
    float *d_w = nullptr; DevList mem_w;
    size_t o_pos_wf = 0, o_pos_g = 0, o_pos_b = 0, o_pos_wd = 0, o_c_wf = 0, o_c_g = 0, o_c_b = 0, o_c_wd = 0;
    std::vector<size_t> o_img, o_g, o_b;
    // workspace (sm_devmem.h: grown by grow() for capP points, freed with the context)
    int64_t capP = 0; DevList mem_P;
    float *h0 = nullptr, *hcat = nullptr, *y = nullptr, *xx = nullptr, *pd = nullptr;
    int *idx = nullptr;
    double *acc = nullptr;
};

namespace {
// the workspace of an encode of P points (the context's; shapemol_se_encode and shapemol_se_train_forward share it)
int se_grow(shapemol_se_ctx *c, int64_t P) {
    const int C = c->C, L = c->L, LAT = c->LAT;
    SMCHK(grow(c->mem_P, {dev_buf(&c->h0, P * C * 3 * 4), dev_buf(&c->hcat, P * L * C * 3 * 4), dev_buf(&c->y, P * 4 * C * 3 * 4), dev_buf(&c->xx, P * 4),
                          dev_buf(&c->pd, P * (LAT + 1) * 3 * 4), dev_buf(&c->idx, P * kSeK * 4), dev_buf(&c->acc, (size_t)kSeReplicas * 2 * 256 * 8)},
               c->capP, P));
    return 0;
}

// the caller's workspace of a training call on P points: byte offsets of its parts, and the split geometry of the two weight products
struct SeTrainWs {
    size_t y, dY, dhcat, dh0, gpd, deg, rowptr, rev, part, S, wT, pw, total;
    int parts, n_groups, dw_splits, dw_per, head_splits, head_per;
};
SeTrainWs se_train_ws(const shapemol_se_ctx *c, int64_t P) {
    const size_t C = c->C, L = c->L, LAT = c->LAT, p = (size_t)P;
    SeTrainWs w{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~size_t(255); return at; };
    w.parts = (int)(P < kSeParts ? P : kSeParts);
    w.n_groups = (int)(P / 16);
    int s = w.n_groups / 8; s = s < 1 ? 1 : (s > kSeDwMaxSplits ? kSeDwMaxSplits : s);
    w.dw_per = (w.n_groups + s - 1) / s; w.dw_splits = (w.n_groups + w.dw_per - 1) / w.dw_per;
    int hs = (int)(P / 128); hs = hs < 1 ? 1 : (hs > 32 ? 32 : hs);
    w.head_per = (int)((P + hs - 1) / hs); w.head_splits = (int)((P + w.head_per - 1) / w.head_per);
    w.y = take(p * 4 * C * 3 * 4); w.dY = take(p * 4 * C * 3 * 4); w.dhcat = take(p * L * C * 3 * 4); w.dh0 = take(p * C * 3 * 4);
    w.gpd = take(p * (LAT + 1) * 3 * 4); w.deg = take(p * 4); w.rowptr = take(p * 4); w.rev = take(p * kSeK * 4);
    w.part = take((size_t)kSeParts * kSePartQ * kSeCh * 8); w.S = take((size_t)kSePartQ * kSeCh * 8); w.wT = take(4 * C * C * 4);
    const size_t pw_edge = (size_t)4 * w.dw_splits * C * C * 4, pw_head = (size_t)w.head_splits * (LAT + 1) * L * C * 8;
    w.pw = take(pw_edge > pw_head ? pw_edge : pw_head);
    w.total = o;
    return w;
}

// the shape limits of an encode, for every call that takes a batch of clouds
int se_check_shape(const shapemol_se_ctx *c, const char *who, int64_t B, int64_t N) {
    if (B < 1 || B > 65535 || N < 32 || (N % 16) != 0 || N > c->max_n || B * N > (1 << 24))
        return sm_fail(std::string(who) + ": need 1 <= B <= 65535, N a multiple of 16 in [32, " + std::to_string(c->max_n) + "] (16 * N * 4 bytes of the " +
                       std::to_string(c->lds_limit) + " bytes of LDS a workgroup can have on this device) and B * N <= 2^24; got B = " +
                       std::to_string(B) + ", N = " + std::to_string(N));
    return 0;
}
int se_check_ws(const SeTrainWs &w, const char *who, const void *d_ws, size_t ws_bytes) {
    if (!d_ws || ((uintptr_t)d_ws & 255) != 0) return sm_fail(std::string(who) + ": the workspace must be a device buffer aligned to 256 bytes");
    if (ws_bytes < w.total)
        return sm_fail(std::string(who) + ": the workspace has " + std::to_string(ws_bytes) + " bytes, shapemol_se_train_workspace asks for " + std::to_string(w.total));
    return 0;
}

// Where a forward sweep leaves its results, and how it takes the batch sums of its L + 2 stages (0: conv_pos, l + 1: block l, L + 1: conv_c)
struct SeForwardDst {
    int *idx; size_t idx_stride;    // neighbour lists: stage l's [P][k] at idx + l * idx_stride (stride 0: one list, every stage overwrites it)
    float *h0, *hcat, *pd;
    float *out;                     // null: the sweep ends after its blocks, conv_c does not run
    double *part, *stats;           // part null: replicated float64 atomics.  Else fixed-order partials [kSeParts][kSePartQ][kSeCh], and the
};                                  // stages' mean and variance go to stats [L + 2][2][kSeCh]

// The batch sums of ||p|| of one edge stage into the context's accumulator: the one place that knows the two modes of an edge stage
template <bool L0>
int se_edge_stats(shapemol_se_ctx *c, hipStream_t s, const SeEdgeArgs &e, const SeForwardDst &dst, int stage) {
    if (!dst.part) {
        SMCHK(hipMemsetAsync(c->acc, 0, (size_t)kSeReplicas * 2 * 256 * 8, s));
        hipLaunchKernelGGL(se_edge_stats_kernel<L0>, dim3((unsigned)e.n_total), dim3(e.C), 0, s, e);
    } else {
        const int parts = e.n_total < kSeParts ? e.n_total : kSeParts;
        hipLaunchKernelGGL(se_edge_stats_part_kernel<L0>, dim3(parts), dim3(e.C), 0, s, e, dst.part);
        hipLaunchKernelGGL(se_stats_reduce_kernel, dim3(1), dim3(256), 0, s, dst.part, parts, e.C, (double)e.n_total * kSeK, c->acc, dst.stats + (size_t)stage * 2 * kSeCh);
    }
    return 0;
}

// The forward sweep on B clouds of N points (checked by the caller): kNN, conv_pos, n_blocks x (squared norms, kNN, point product,
// batch sums, apply), and conv_c with the mean over the points where dst.out is given.  xx, y and the accumulator are the context's
// (se_grow for B * N points has run).  n_blocks and dst.out are the caller's: shapemol_se_debug_stop_after shortens
// shapemol_se_encode alone, a training forward always passes L blocks and its output.
int se_forward(shapemol_se_ctx *c, hipStream_t s, const float *d_points, int64_t B, int64_t N, const SeForwardDst &dst, int n_blocks) {
    const int C = c->C, L = c->L, LAT = c->LAT;
    const int64_t P = B * N;
    const size_t knn_lds = (size_t)16 * N * sizeof(float);      // <= lds_limit (N <= max_n)
    SMCHK(hipFuncSetAttribute((const void *)se_knn_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)knn_lds));
    SMCHK(hipFuncSetAttribute((const void *)se_knn_kernel<3 * kC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)knn_lds));
    const float *W = c->d_w;
    const dim3 knn_grid((unsigned)(N / 16), (unsigned)B);
    auto stage_idx = [&](int stage) { return dst.idx + stage * dst.idx_stride; };
    auto edge_args = [&](int stage, const float *bn_g, const float *bn_b, float *h_out, int h_ld, int h_off) {
        SeEdgeArgs e{};
        e.x = d_points; e.w0f = W + c->o_pos_wf; e.w0d = W + c->o_pos_wd; e.y = c->y;      // (conv_pos reads x and w0, a block y)
        e.idx = stage_idx(stage); e.bn_g = bn_g; e.bn_b = bn_b; e.acc = c->acc; e.h_out = h_out;
        e.n_total = (int)P; e.N = (int)N; e.C = C; e.h_ld = h_ld; e.h_off = h_off;
        return e;
    };
    // conv_pos on the raw points
    const SeEdgeArgs e = edge_args(0, W + c->o_pos_g, W + c->o_pos_b, dst.h0, 3 * C, 0);
    hipLaunchKernelGGL(se_knn_kernel<3>, knn_grid, dim3(256), knn_lds, s, d_points, 3, nullptr, (int)N, stage_idx(0));
    if (se_edge_stats<true>(c, s, e, dst, 0)) return 1;
    hipLaunchKernelGGL(se_edge_apply_kernel<true>, dim3((unsigned)P), dim3(C), 0, s, e);
    // DGCNN blocks
    for (int l = 0; l < n_blocks; ++l) {
        const float *hin = l == 0 ? dst.h0 : dst.hcat + (size_t)(l - 1) * 3 * C;
        const int ld = l == 0 ? 3 * C : L * 3 * C;
        const SeEdgeArgs b = edge_args(l + 1, W + c->o_g[l], W + c->o_b[l], dst.hcat, L * 3 * C, l * 3 * C);
        hipLaunchKernelGGL(se_sqnorm_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, s, hin, (int)P, 3 * C, ld, c->xx);
        hipLaunchKernelGGL(se_knn_kernel<3 * kC>, knn_grid, dim3(256), knn_lds, s, hin, ld, c->xx, (int)N, stage_idx(l + 1));
        hipLaunchKernelGGL(se_point_linear_kernel<kC>, dim3((unsigned)((P * 3 + 15) / 16)), dim3(256), 0, s, hin, ld, W + c->o_img[l], (int)(P * 3), 4 * C, c->y);
        if (se_edge_stats<false>(c, s, b, dst, l + 1)) return 1;
        hipLaunchKernelGGL(se_edge_apply_kernel<false>, dim3((unsigned)P), dim3(C), 0, s, b);
    }
    if (dst.out) {
        // conv_c + mean over the points.  se_head_linear_kernel adds its sums into the accumulator in both modes; with partials the
        // reducer then overwrites them
        SeHeadArgs ha{dst.hcat, W + c->o_c_wf, W + c->o_c_wd, W + c->o_c_g, W + c->o_c_b, dst.pd, c->acc, dst.out, (int)P, (int)N, L * C, LAT};
        SMCHK(hipMemsetAsync(c->acc, 0, (size_t)kSeReplicas * 2 * 256 * 8, s));
        hipLaunchKernelGGL(se_head_linear_kernel, dim3((unsigned)((P * (LAT + 1) + 3) / 4)), dim3(256), 0, s, ha);
        if (dst.part) {
            const int parts = (int)(P < kSeParts ? P : kSeParts);
            hipLaunchKernelGGL(se_head_stats_part_kernel, dim3(parts), dim3(256), 0, s, dst.pd, (int)P, LAT, dst.part);
            hipLaunchKernelGGL(se_stats_reduce_kernel, dim3(1), dim3(256), 0, s, dst.part, parts, LAT, (double)P, c->acc, dst.stats + (size_t)(L + 1) * 2 * kSeCh);
        }
        hipLaunchKernelGGL(se_head_apply_kernel, dim3((unsigned)(B * LAT)), dim3(256), 0, s, ha);
    }
    SMCHK(hipGetLastError());
    return 0;
}

// the context's weight image from the flat vector d_flat (DEVICE, the order of shapemol_se_create's weights): one kernel on s
void se_pack_weights(const shapemol_se_ctx *c, const float *d_flat, hipStream_t s) {
    SeLoadArgs a{};
    a.src = d_flat; a.dst = c->d_w; a.L = c->L; a.LAT = c->LAT;
    a.o_pos_wf = (unsigned)c->o_pos_wf; a.o_pos_g = (unsigned)c->o_pos_g; a.o_pos_b = (unsigned)c->o_pos_b; a.o_pos_wd = (unsigned)c->o_pos_wd;
    a.o_c_wf = (unsigned)c->o_c_wf; a.o_c_g = (unsigned)c->o_c_g; a.o_c_b = (unsigned)c->o_c_b; a.o_c_wd = (unsigned)c->o_c_wd;
    for (int l = 0; l < c->L; ++l) { a.o_img[l] = (unsigned)c->o_img[l]; a.o_g[l] = (unsigned)c->o_g[l]; a.o_b[l] = (unsigned)c->o_b[l]; }
    hipLaunchKernelGGL(se_load_weights_kernel, dim3((unsigned)((shapemol_se_weight_count(c->C, c->LAT, c->L) + 255) / 256)), dim3(256), 0, s, a);
}
}  // namespace

extern "C" {

size_t shapemol_se_weight_count(int32_t hidden_dim, int32_t latent_dim, int32_t layer_num) {
    const size_t C = hidden_dim, LAT = latent_dim, L = layer_num;
    return (2 * C + 2 * C + 2 * C) + L * (2 * C * C + 2 * C + 2 * C * C) + (LAT * L * C + 2 * LAT + L * C);
}

int shapemol_se_create(int32_t hidden_dim, int32_t latent_dim, int32_t layer_num, int32_t num_k, const float *w, size_t n_weights,
                       int device, shapemol_se_ctx **out) {
    if (!w || !out) return sm_fail("shapemol_se_create: null argument");
    if (hidden_dim != kC) return sm_fail("shapemol_se_create: hidden_dim must be 128");
    if (num_k != kSeK) return sm_fail("shapemol_se_create: num_k must be 20");
    if (latent_dim < 1 || latent_dim > 256 || layer_num < 1 || layer_num > 8) return sm_fail("shapemol_se_create: latent_dim / layer_num out of range");
    if (n_weights != shapemol_se_weight_count(hidden_dim, latent_dim, layer_num)) return sm_fail("shapemol_se_create: weight count mismatch");
    if (sm_open_device(device, "shapemol_se_create")) return 1;
    // se_knn_kernel keeps the 16 x N distances of its row block in dynamic LDS: the device's limit per workgroup bounds N
    int lds = 0;
    SMCHK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    const int max_n = lds / (16 * (int)sizeof(float)) / 16 * 16;
    if (max_n < 32) return sm_fail("shapemol_se_create: the device has less than 2 KB of LDS per workgroup");
    auto *c = new shapemol_se_ctx();
    c->LAT = latent_dim; c->L = layer_num; c->device = device; c->lds_limit = lds; c->max_n = max_n;
    // the image's parts, each at a multiple of 64 floats: plain copies of the flat vector's, and per block the A fragments of
    // W' = [Wf1 ; Wf2 - Wf1 ; Wd1 ; Wd2 - Wd1] (4C x C) for se_point_linear_kernel.  se_pack_weights fills it
    const size_t C = kC, L = layer_num, LAT = latent_dim;
    size_t n_img = 0;
    auto take = [&](size_t n) { const size_t o = (n_img + 63) & ~size_t(63); n_img = o + n; return o; };
    c->o_pos_wf = take(2 * C); c->o_pos_g = take(C); c->o_pos_b = take(C); c->o_pos_wd = take(2 * C);
    for (size_t l = 0; l < L; ++l) { c->o_g.push_back(take(C)); c->o_b.push_back(take(C)); c->o_img.push_back(take(4 * C * C)); }
    c->o_c_wf = take(LAT * L * C); c->o_c_g = take(LAT); c->o_c_b = take(LAT); c->o_c_wd = take(L * C);
    float *stage = nullptr;
    DevList mem_stage;                                                          // (freed when this function returns)
    hipError_t e = c->mem_w.alloc(&c->d_w, n_img * 4, true);                    // (zeroed: the alignment gaps behind conv_c's bn vectors)
    if (e == hipSuccess) e = mem_stage.alloc(&stage, n_weights * 4);
    if (e == hipSuccess) e = hipMemcpy(stage, w, n_weights * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) { se_pack_weights(c, stage, nullptr); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        delete c; return sm_fail(std::string("shapemol_se_create: device allocation failed: ") + hipGetErrorString(e));
    }
    *out = c;
    return 0;
}

void shapemol_se_destroy(shapemol_se_ctx *c) {
    if (!c) return;
    sm_close_device(c->device);
    delete c;                // its lists release what they own
}

int shapemol_se_encode(shapemol_se_ctx *c, const float *d_points, int64_t B, int64_t N, float *d_out, void *stream) {
    if (!c || !d_points || !d_out) return sm_fail("shapemol_se_encode: null argument");
    if (se_check_shape(c, "shapemol_se_encode", B, N)) return 1;
    SMCHK(hipSetDevice(c->device));
    if (se_grow(c, B * N)) return 1;
    c->lastP = B * N;
    // into the context's workspace (shapemol_se_debug_read reads it), one neighbour list, atomic sums; shapemol_se_debug_stop_after
    // ends the sweep after its blocks and leaves d_out alone
    const bool stop = c->stop_after >= 0;
    const SeForwardDst dst{c->idx, 0, c->h0, c->hcat, c->pd, stop ? nullptr : d_out, nullptr, nullptr};
    return se_forward(c, (hipStream_t)stream, d_points, B, N, dst, stop ? c->stop_after : c->L);
}

int64_t shapemol_se_max_points(const shapemol_se_ctx *c) { return c ? c->max_n : 0; }

int shapemol_se_load_weights(shapemol_se_ctx *c, const float *d_weights, size_t n_weights, void *stream) {
    if (!c || !d_weights) return sm_fail("shapemol_se_load_weights: null argument");
    if (n_weights != shapemol_se_weight_count(c->C, c->LAT, c->L))
        return sm_fail("shapemol_se_load_weights: weight count mismatch: the context holds " + std::to_string(shapemol_se_weight_count(c->C, c->LAT, c->L)) +
                       " weights, got " + std::to_string(n_weights));
    SMCHK(hipSetDevice(c->device));
    se_pack_weights(c, d_weights, (hipStream_t)stream);
    SMCHK(hipGetLastError());
    return 0;
}

size_t shapemol_se_train_workspace(const shapemol_se_ctx *c, int64_t B, int64_t N) {
    if (!c || B < 1 || N < 1 || B * N > (1 << 24)) return 0;
    return se_train_ws(c, B * N).total;
}

int shapemol_se_train_forward(shapemol_se_ctx *c, const float *d_points, int64_t B, int64_t N, int32_t *d_idx, float *d_h0, float *d_hcat,
                              double *d_stats, float *d_pd, float *d_out, void *d_ws, size_t ws_bytes, void *stream) {
    const char *who = "shapemol_se_train_forward";
    if (!c || !d_points || !d_idx || !d_h0 || !d_hcat || !d_stats || !d_pd || !d_out) return sm_fail(std::string(who) + ": null argument");
    if (se_check_shape(c, who, B, N)) return 1;
    const int64_t P = B * N;
    const SeTrainWs ws = se_train_ws(c, P);
    if (se_check_ws(ws, who, d_ws, ws_bytes)) return 1;
    SMCHK(hipSetDevice(c->device));
    if (se_grow(c, P)) return 1;
    // into the caller's tensors, a neighbour list per stage, fixed-order sums; always the full sweep (shapemol_se_debug_stop_after is shapemol_se_encode's)
    const SeForwardDst dst{d_idx, (size_t)P * kSeK, d_h0, d_hcat, d_pd, d_out, (double *)((char *)d_ws + ws.part), d_stats};
    return se_forward(c, (hipStream_t)stream, d_points, B, N, dst, c->L);
}

int shapemol_se_train_backward(shapemol_se_ctx *c, const float *d_points, int64_t B, int64_t N, const int32_t *d_idx, const float *d_h0,
                               const float *d_hcat, const double *d_stats, const float *d_pd, const float *d_grad_out, const float *d_grad_hcat,
                               float *d_grad_w, int32_t *d_masks, void *d_ws, size_t ws_bytes, void *stream) {
    const char *who = "shapemol_se_train_backward";
    if (!c || !d_points || !d_idx || !d_h0 || !d_hcat || !d_stats || !d_pd || !d_grad_w) return sm_fail(std::string(who) + ": null argument");
    if ((d_grad_out == nullptr) == (d_grad_hcat == nullptr)) return sm_fail(std::string(who) + ": give the latent's gradient or hcat's, not both");
    if (se_check_shape(c, who, B, N)) return 1;
    const int64_t P = B * N;
    const SeTrainWs ws = se_train_ws(c, P);
    if (se_check_ws(ws, who, d_ws, ws_bytes)) return 1;
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int C = c->C, L = c->L, LAT = c->LAT, KC = L * C;
    char *wb = (char *)d_ws;
    float *y = (float *)(wb + ws.y), *dY = (float *)(wb + ws.dY), *dhcat = (float *)(wb + ws.dhcat), *dh0 = (float *)(wb + ws.dh0), *gpd = (float *)(wb + ws.gpd);
    int *deg = (int *)(wb + ws.deg), *rowptr = (int *)(wb + ws.rowptr), *rev = (int *)(wb + ws.rev);
    double *part = (double *)(wb + ws.part), *S = (double *)(wb + ws.S);
    float *wT = (float *)(wb + ws.wT), *pw = (float *)(wb + ws.pw);
    const float *W = c->d_w;
    // the gradient vector, in the weights' order
    const size_t blk = (size_t)4 * C * C + 2 * C, n_cwf = (size_t)LAT * KC;
    float *g_pos = d_grad_w, *g_blocks = d_grad_w + 6 * C, *g_c = g_blocks + L * blk;
    const double *st_c = d_stats + (size_t)(L + 1) * 2 * kSeCh;
    if (d_grad_hcat) {
        SMCHK(hipMemcpyAsync(dhcat, d_grad_hcat, (size_t)P * KC * 3 * 4, hipMemcpyDeviceToDevice, s));
        SMCHK(hipMemsetAsync(g_c, 0, (n_cwf + 2 * LAT + KC) * 4, s));
    } else {
        SeHeadBwdArgs hb{d_hcat, W + c->o_c_wf, W + c->o_c_wd, W + c->o_c_g, W + c->o_c_b, d_pd, st_c, S, d_grad_out, gpd, dhcat,
                         d_masks ? d_masks + (size_t)(L + 1) * P * kSeCh : nullptr, (int)P, (int)N, KC, LAT};
        hipLaunchKernelGGL(se_head_bwd_sums_kernel, dim3(ws.parts), dim3(256), 0, s, hb, part);
        SeSumDst o{};
        o.dst[0] = g_c + n_cwf + LAT; o.stride[0] = 1; o.dst[1] = g_c + n_cwf; o.stride[1] = 1;          // S1 = dbeta, S2 = dgamma
        hipLaunchKernelGGL(se_part_reduce_kernel, dim3(2), dim3(256), 0, s, part, ws.parts, 2, LAT, S, o);
        hipLaunchKernelGGL(se_head_bwd_point_kernel, dim3((unsigned)P), dim3(256), 0, s, hb);
        const unsigned eb = (unsigned)(((size_t)(LAT + 1) * KC + 255) / 256);
        hipLaunchKernelGGL(se_head_bwd_dw_kernel, dim3(eb, ws.head_splits), dim3(256), 0, s, hb, ws.head_per, (double *)pw);
        hipLaunchKernelGGL(se_head_bwd_dw_finish_kernel, dim3(eb), dim3(256), 0, s, (const double *)pw, ws.head_splits, LAT, KC, g_c, g_c + n_cwf + 2 * LAT);
    }
    for (int l = L - 1; l >= 0; --l) {
        const float *hin = l == 0 ? d_h0 : d_hcat + (size_t)(l - 1) * 3 * C;
        const int ld = l == 0 ? 3 * C : L * 3 * C;
        const int32_t *idx = d_idx + (size_t)(l + 1) * P * kSeK;
        float *gl = g_blocks + l * blk;
        SMCHK(hipMemsetAsync(deg, 0, (size_t)P * 4, s));
        hipLaunchKernelGGL(se_deg_kernel, dim3((unsigned)((P * kSeK + 255) / 256)), dim3(256), 0, s, idx, (int)P, (int)N, deg);
        hipLaunchKernelGGL(se_rowptr_kernel, dim3((unsigned)B), dim3(256), 0, s, deg, (int)N, rowptr);
        hipLaunchKernelGGL(se_rev_fill_kernel, dim3((unsigned)(N / 16), (unsigned)B), dim3(256), 0, s, idx, (int)N, rowptr, rev);
        hipLaunchKernelGGL(se_point_linear_kernel<kC>, dim3((unsigned)((P * 3 + 15) / 16)), dim3(256), 0, s, hin, ld, W + c->o_img[l], (int)(P * 3), 4 * C, y);
        SeBwdArgs a{};
        a.e.y = y; a.e.idx = idx; a.e.bn_g = W + c->o_g[l]; a.e.bn_b = W + c->o_b[l]; a.e.n_total = (int)P; a.e.N = (int)N; a.e.C = C;
        a.stats = d_stats + (size_t)(l + 1) * 2 * kSeCh; a.dH = dhcat; a.dh_ld = L * 3 * C; a.dh_off = l * 3 * C;
        a.deg = deg; a.rowptr = rowptr; a.rev = rev; a.dY = dY; a.mask = d_masks ? d_masks + (size_t)(l + 1) * P * kSeCh : nullptr;
        hipLaunchKernelGGL((se_edge_bwd_sums_kernel<false, 0>), dim3(ws.parts), dim3(C), 0, s, a, part);
        SeSumDst o{};
        o.dst[0] = gl + 2 * C * C + C; o.stride[0] = 1; o.dst[1] = gl + 2 * C * C; o.stride[1] = 1;
        hipLaunchKernelGGL(se_part_reduce_kernel, dim3(2), dim3(256), 0, s, part, ws.parts, 2, C, S, o);
        a.S = S;
        hipLaunchKernelGGL(se_edge_bwd_gather_kernel, dim3((unsigned)P), dim3(C), 0, s, a);
        hipLaunchKernelGGL(se_wimg_transpose_kernel<kC>, dim3(4 * C * C / 256), dim3(256), 0, s, W + c->o_img[l], wT);
        hipLaunchKernelGGL(se_dhin_kernel<kC>, dim3((unsigned)((P * 3 + 15) / 16)), dim3(256), 0, s, dY, wT, (int)(P * 3), l == 0 ? dh0 : dhcat,
                           l == 0 ? 3 * C : L * 3 * C, l == 0 ? 0 : (l - 1) * 3 * C, l == 0 ? 0 : 1);
        hipLaunchKernelGGL(se_dw_kernel, dim3(4, ws.dw_splits), dim3(256), 0, s, dY, hin, ld, ws.n_groups, ws.dw_per, pw);
        hipLaunchKernelGGL(se_dw_finish_kernel, dim3(C * C / 256), dim3(256), 0, s, pw, ws.dw_splits, gl, gl + 2 * C * C + 2 * C);
    }
    {   // conv_pos: one input channel, its weight gradients are direct sums over the edges
        SeBwdArgs a{};
        a.e.x = d_points; a.e.w0f = W + c->o_pos_wf; a.e.w0d = W + c->o_pos_wd; a.e.idx = d_idx; a.e.bn_g = W + c->o_pos_g; a.e.bn_b = W + c->o_pos_b;
        a.e.n_total = (int)P; a.e.N = (int)N; a.e.C = C;
        a.stats = d_stats; a.dH = dh0; a.dh_ld = 3 * C; a.dh_off = 0; a.mask = d_masks;
        hipLaunchKernelGGL((se_edge_bwd_sums_kernel<true, 0>), dim3(ws.parts), dim3(C), 0, s, a, part);
        SeSumDst o{};
        o.dst[0] = g_pos + 3 * C; o.stride[0] = 1; o.dst[1] = g_pos + 2 * C; o.stride[1] = 1;
        hipLaunchKernelGGL(se_part_reduce_kernel, dim3(2), dim3(256), 0, s, part, ws.parts, 2, C, S, o);
        a.S = S;
        hipLaunchKernelGGL((se_edge_bwd_sums_kernel<true, 1>), dim3(ws.parts), dim3(C), 0, s, a, part);
        SeSumDst w{};
        w.dst[0] = g_pos; w.dst[1] = g_pos + 1; w.dst[2] = g_pos + 4 * C; w.dst[3] = g_pos + 4 * C + 1;
        w.stride[0] = w.stride[1] = w.stride[2] = w.stride[3] = 2;
        hipLaunchKernelGGL(se_part_reduce_kernel, dim3(4), dim3(256), 0, s, part, ws.parts, 4, C, S + 2 * kSeCh, w);
    }
    SMCHK(hipGetLastError());
    return 0;
}

int shapemol_se_debug_stop_after(shapemol_se_ctx *c, int32_t n_blocks) {
    if (!c) return sm_fail("shapemol_se_debug_stop_after: null argument");
    if (n_blocks < -1 || n_blocks > c->L) return sm_fail("shapemol_se_debug_stop_after: n_blocks must be -1 (off) or in [0, layer_num]");
    c->stop_after = n_blocks;
    return 0;
}

int shapemol_se_debug_read(shapemol_se_ctx *c, int32_t what, void *h_dst, size_t n_bytes) {
    if (!c || !h_dst) return sm_fail("shapemol_se_debug_read: null argument");
    if (c->lastP == 0) return sm_fail("shapemol_se_debug_read: no shapemol_se_encode has run on this context");
    const size_t P = (size_t)c->lastP, C = c->C, L = c->L, LAT = c->LAT;
    const void *src = nullptr; size_t need = 0;
    switch (what) {
        case SHAPEMOL_SE_IDX:  src = c->idx;  need = P * kSeK * 4; break;
        case SHAPEMOL_SE_H0:   src = c->h0;   need = P * C * 3 * 4; break;
        case SHAPEMOL_SE_HCAT: src = c->hcat; need = P * L * C * 3 * 4; break;
        case SHAPEMOL_SE_Y:    src = c->y;    need = P * 4 * C * 3 * 4; break;
        case SHAPEMOL_SE_XX:   src = c->xx;   need = P * 4; break;
        case SHAPEMOL_SE_PD:   src = c->pd;   need = P * (LAT + 1) * 3 * 4; break;
        default: return sm_fail("shapemol_se_debug_read: what must be one of SHAPEMOL_SE_IDX .. SHAPEMOL_SE_PD (0 .. 5), got " + std::to_string(what));
    }
    if (n_bytes != need) return sm_fail("shapemol_se_debug_read: buffer " + std::to_string(what) + " of the last encode has " + std::to_string(need) + " bytes, n_bytes is " + std::to_string(n_bytes));
    SMCHK(hipSetDevice(c->device));
    SMCHK(hipDeviceSynchronize());
    SMCHK(hipMemcpy(h_dst, src, need, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
