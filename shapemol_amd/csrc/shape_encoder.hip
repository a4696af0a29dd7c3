// C ABI of the device shape encoder (include/shapemol_hip.h, shapemol_se_*): VN_DGCNN_Encoder.forward of the reference
// (models/shape_pointcloud_modelAE.py:207-255).  Kernels: sm_shape.h.
#include "../../include/shapemol_hip.h"
#include "sm_shape.h"
#include "sm_devmem.h"
#include "sm_host.h"

#include <cstring>
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
    const int C = kC;
    std::vector<float> img;
    auto put = [&](const float *src, size_t n) { const size_t o = (img.size() + 63) & ~size_t(63); img.resize(o + n); std::memcpy(&img[o], src, n * 4); return o; };
    const float *p = w;
    c->o_pos_wf = put(p, 2 * C); p += 2 * C;
    c->o_pos_g = put(p, C); p += C;
    c->o_pos_b = put(p, C); p += C;
    c->o_pos_wd = put(p, 2 * C); p += 2 * C;
    for (int l = 0; l < layer_num; ++l) {
        const float *wf = p; p += (size_t)C * 2 * C;
        c->o_g.push_back(put(p, C)); p += C;
        c->o_b.push_back(put(p, C)); p += C;
        const float *wd = p; p += (size_t)C * 2 * C;
        // W' = [Wf1 ; Wf2 - Wf1 ; Wd1 ; Wd2 - Wd1]  (4C x C), as A fragments of se_point_linear_kernel
        std::vector<float> Wp((size_t)4 * C * C);
        for (int m = 0; m < C; ++m)
            for (int k = 0; k < C; ++k) {
                Wp[(size_t)(0 * C + m) * C + k] = wf[(size_t)m * 2 * C + k];
                Wp[(size_t)(1 * C + m) * C + k] = wf[(size_t)m * 2 * C + C + k] - wf[(size_t)m * 2 * C + k];
                Wp[(size_t)(2 * C + m) * C + k] = wd[(size_t)m * 2 * C + k];
                Wp[(size_t)(3 * C + m) * C + k] = wd[(size_t)m * 2 * C + C + k] - wd[(size_t)m * 2 * C + k];
            }
        std::vector<float> im((size_t)4 * C * C);
        for (int t = 0; t < 4 * C / 16; ++t)
            for (int s4 = 0; s4 < C / 16; ++s4)
                for (int lane = 0; lane < 64; ++lane)
                    for (int r = 0; r < 4; ++r)
                        im[((size_t)(t * (C / 16) + s4) * 64 + lane) * 4 + r] = Wp[(size_t)(16 * t + (lane & 15)) * C + 4 * (4 * s4 + r) + (lane >> 4)];
        c->o_img.push_back(put(im.data(), im.size()));
    }
    c->o_c_wf = put(p, (size_t)latent_dim * layer_num * C); p += (size_t)latent_dim * layer_num * C;
    c->o_c_g = put(p, latent_dim); p += latent_dim;
    c->o_c_b = put(p, latent_dim); p += latent_dim;
    c->o_c_wd = put(p, (size_t)layer_num * C); p += (size_t)layer_num * C;
    if (c->mem_w.alloc(&c->d_w, img.size() * 4) != hipSuccess || hipMemcpy(c->d_w, img.data(), img.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        delete c; return sm_fail("shapemol_se_create: device allocation failed");
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
    if (B < 1 || B > 65535 || N < 32 || (N % 16) != 0 || N > c->max_n || B * N > (1 << 24))
        return sm_fail("shapemol_se_encode: need 1 <= B <= 65535, N a multiple of 16 in [32, " + std::to_string(c->max_n) + "] (16 * N * 4 bytes of the " +
                       std::to_string(c->lds_limit) + " bytes of LDS a workgroup can have on this device) and B * N <= 2^24; got B = " +
                       std::to_string(B) + ", N = " + std::to_string(N));
    SMCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int C = c->C, L = c->L, LAT = c->LAT;
    const int64_t P = B * N;
    SMCHK(grow(c->mem_P, {dev_buf(&c->h0, P * C * 3 * 4), dev_buf(&c->hcat, P * L * C * 3 * 4), dev_buf(&c->y, P * 4 * C * 3 * 4), dev_buf(&c->xx, P * 4),
                          dev_buf(&c->pd, P * (LAT + 1) * 3 * 4), dev_buf(&c->idx, P * kSeK * 4), dev_buf(&c->acc, (size_t)kSeReplicas * 2 * 256 * 8)},
               c->capP, P));
    c->lastP = P;
    const size_t knn_lds = (size_t)16 * N * sizeof(float);      // <= lds_limit (N <= max_n)
    SMCHK(hipFuncSetAttribute((const void *)se_knn_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)knn_lds));
    SMCHK(hipFuncSetAttribute((const void *)se_knn_kernel<3 * kC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)knn_lds));
    const int n_blocks = c->stop_after < 0 ? L : (c->stop_after < L ? c->stop_after : L);
    const float *W = c->d_w;
    const dim3 knn_grid((unsigned)(N / 16), (unsigned)B);
    // conv_pos on the raw points
    hipLaunchKernelGGL(se_knn_kernel<3>, knn_grid, dim3(256), knn_lds, s, d_points, 3, nullptr, (int)N, c->idx);
    SeEdgeArgs e{};
    e.x = d_points; e.w0f = W + c->o_pos_wf; e.w0d = W + c->o_pos_wd; e.idx = c->idx; e.bn_g = W + c->o_pos_g; e.bn_b = W + c->o_pos_b;
    e.acc = c->acc; e.h_out = c->h0; e.n_total = (int)P; e.N = (int)N; e.C = C; e.h_ld = 3 * C; e.h_off = 0;
    SMCHK(hipMemsetAsync(c->acc, 0, (size_t)kSeReplicas * 2 * 256 * 8, s));
    hipLaunchKernelGGL(se_edge_stats_kernel<true>, dim3((unsigned)P), dim3(C), 0, s, e);
    hipLaunchKernelGGL(se_edge_apply_kernel<true>, dim3((unsigned)P), dim3(C), 0, s, e);
    // DGCNN blocks
    for (int l = 0; l < n_blocks; ++l) {
        const float *hin = l == 0 ? c->h0 : c->hcat + (size_t)(l - 1) * 3 * C;
        const int ld = l == 0 ? 3 * C : L * 3 * C;
        hipLaunchKernelGGL(se_sqnorm_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, s, hin, (int)P, 3 * C, ld, c->xx);
        hipLaunchKernelGGL(se_knn_kernel<3 * kC>, knn_grid, dim3(256), knn_lds, s, hin, ld, c->xx, (int)N, c->idx);
        hipLaunchKernelGGL(se_point_linear_kernel<kC>, dim3((unsigned)((P * 3 + 15) / 16)), dim3(256), 0, s, hin, ld, W + c->o_img[l], (int)(P * 3), 4 * C, c->y);
        SeEdgeArgs b{};
        b.y = c->y; b.idx = c->idx; b.bn_g = W + c->o_g[l]; b.bn_b = W + c->o_b[l]; b.acc = c->acc; b.h_out = c->hcat;
        b.n_total = (int)P; b.N = (int)N; b.C = C; b.h_ld = L * 3 * C; b.h_off = l * 3 * C;
        SMCHK(hipMemsetAsync(c->acc, 0, (size_t)kSeReplicas * 2 * 256 * 8, s));
        hipLaunchKernelGGL(se_edge_stats_kernel<false>, dim3((unsigned)P), dim3(C), 0, s, b);
        hipLaunchKernelGGL(se_edge_apply_kernel<false>, dim3((unsigned)P), dim3(C), 0, s, b);
    }
    if (c->stop_after >= 0) { SMCHK(hipGetLastError()); return 0; }
    // conv_c + mean over the points
    SeHeadArgs ha{c->hcat, W + c->o_c_wf, W + c->o_c_wd, W + c->o_c_g, W + c->o_c_b, c->pd, c->acc, d_out, (int)P, (int)N, L * C, LAT};
    SMCHK(hipMemsetAsync(c->acc, 0, (size_t)kSeReplicas * 2 * 256 * 8, s));
    hipLaunchKernelGGL(se_head_linear_kernel, dim3((unsigned)((P * (LAT + 1) + 3) / 4)), dim3(256), 0, s, ha);
    hipLaunchKernelGGL(se_head_apply_kernel, dim3((unsigned)(B * LAT)), dim3(256), 0, s, ha);
    SMCHK(hipGetLastError());
    return 0;
}

int64_t shapemol_se_max_points(const shapemol_se_ctx *c) { return c ? c->max_n : 0; }

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
