// C ABI of the device shape decoder (include/shapemol_hip.h, shapemol_sd_*): DecoderInner.forward of the reference
// (models/shape_pointcloud_modelAE.py:21-103).  Kernels: sm_shape_dec.h.
#include "../../include/shapemol_hip.h"
#include "sm_shape_dec.h"

#include <cstring>
#include <string>
#include <vector>

extern "C" void shapemol_set_error_(const char *msg);     // shapemol_hip.hip: stores the thread's last error

namespace {
int sd_fail(const std::string &m) { shapemol_set_error_(m.c_str()); return 1; }
#define SDCHK(expr)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return sd_fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
constexpr int kMaxLatent = 256, kMaxLayers = 8, kMaxShapes = 65535;
}  // namespace

struct shapemol_sd_ctx {
    int Z = 32, L = 4, sigmoid = 0, device = 0, n_cu = 1;
    size_t lds_bytes = 0;
    float *d_w = nullptr;
    size_t o_zin = 0, o_win = 0, o_bin = 0, o_w0 = 0, o_img = 0, o_bias = 0, o_out = 0;
    // per-shape workspace of the prologue: rewritten by every decode, so a context serves one stream at a time
    int64_t capB = 0, lastB = 0;
    float *zinv = nullptr, *gc = nullptr;
};

extern "C" {

size_t shapemol_sd_weight_count(int32_t hidden, int32_t latent, int32_t layer_num) {
    const size_t H = hidden, Z = latent, L = layer_num;
    return Z * Z + H * (2 * Z + 1) + H + L * (2 * H * H + 2 * H) + H + 1;
}

int shapemol_sd_create(int32_t hidden, int32_t latent, int32_t layer_num, int32_t loss_type, const float *w, size_t n_weights,
                       int device, shapemol_sd_ctx **out) {
    if (!w || !out) return sd_fail("shapemol_sd_create: null argument");
    if (hidden != kSdH) return sd_fail("shapemol_sd_create: hidden must be 128, got " + std::to_string(hidden));
    if (latent < 1 || latent > kMaxLatent) return sd_fail("shapemol_sd_create: latent must be in 1..256, got " + std::to_string(latent));
    if (layer_num < 1 || layer_num > kMaxLayers) return sd_fail("shapemol_sd_create: layer_num must be in 1..8, got " + std::to_string(layer_num));
    if (loss_type != SHAPEMOL_SD_SIGNEDDIST && loss_type != SHAPEMOL_SD_OCCUPANCY)
        return sd_fail("shapemol_sd_create: loss_type must be SHAPEMOL_SD_SIGNEDDIST (0) or SHAPEMOL_SD_OCCUPANCY (1), got " + std::to_string(loss_type));
    const size_t need = shapemol_sd_weight_count(hidden, latent, layer_num);
    if (n_weights != need)
        return sd_fail("shapemol_sd_create: weight count mismatch: " + std::to_string(n_weights) + " given, " + std::to_string(need) + " needed");
    int ndev = 0;
    SDCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return sd_fail("shapemol_sd_create: no such HIP device");
    SDCHK(hipSetDevice(device));
    int lds = 0, n_cu = 0;
    SDCHK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    SDCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    const int H = kSdH, Z = latent, L = layer_num;
    const size_t lds_bytes = ((size_t)2 * kSdImg + (size_t)2 * L * H) * sizeof(float);
    if ((size_t)lds < lds_bytes)
        return sd_fail("shapemol_sd_create: the decode kernel needs " + std::to_string(lds_bytes) + " bytes of LDS per workgroup, the device has " + std::to_string(lds));
    // once per context, not per decode; the largest image set (layer_num 8) where it fits, so that contexts of different
    // depths do not shrink each other's limit
    const int lds_all = (int)(((size_t)2 * kSdImg + (size_t)2 * kMaxLayers * H) * sizeof(float));
    SDCHK(hipFuncSetAttribute((const void *)sd_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_all <= lds ? lds_all : (int)lds_bytes));
    auto *c = new shapemol_sd_ctx();
    c->Z = Z; c->L = L; c->sigmoid = loss_type == SHAPEMOL_SD_OCCUPANCY; c->device = device; c->n_cu = n_cu > 0 ? n_cu : 1; c->lds_bytes = lds_bytes;
    std::vector<float> img;
    auto put = [&](const float *src, size_t n) { const size_t o = (img.size() + 63) & ~size_t(63); img.resize(o + n); std::memcpy(&img[o], src, n * 4); return o; };
    const float *p = w;
    c->o_zin = put(p, (size_t)Z * Z); p += (size_t)Z * Z;
    const float *w_in = p;
    c->o_win = put(p, (size_t)H * (2 * Z + 1)); p += (size_t)H * (2 * Z + 1);
    c->o_bin = put(p, H); p += H;
    std::vector<float> w0(H);
    for (int h = 0; h < H; ++h) w0[h] = w_in[(size_t)h * (2 * Z + 1)];
    c->o_w0 = put(w0.data(), H);
    // A fragments of sd_decode_kernel, k in the order of the accumulator layout (sm_shape_dec.h)
    std::vector<float> im((size_t)2 * L * kSdImg), bias((size_t)2 * L * H);
    for (int i = 0; i < 2 * L; ++i) {
        const float *W = p; p += (size_t)H * H;
        std::memcpy(&bias[(size_t)i * H], p, H * 4); p += H;
        for (int to = 0; to < 8; ++to)
            for (int ti = 0; ti < 8; ++ti)
                for (int lane = 0; lane < 64; ++lane)
                    for (int r = 0; r < 4; ++r)
                        im[(size_t)i * kSdImg + ((size_t)(to * 8 + ti) * 64 + lane) * 4 + r] = W[(size_t)(16 * to + (lane & 15)) * H + 16 * ti + 4 * (lane >> 4) + r];
    }
    c->o_img = put(im.data(), im.size());
    c->o_bias = put(bias.data(), bias.size());
    c->o_out = put(p, H + 1); p += H + 1;
    if (hipMalloc((void **)&c->d_w, img.size() * 4) != hipSuccess || hipMemcpy(c->d_w, img.data(), img.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        if (c->d_w) hipFree(c->d_w);
        delete c; return sd_fail("shapemol_sd_create: device allocation failed");
    }
    *out = c;
    return 0;
}

void shapemol_sd_destroy(shapemol_sd_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    for (void *q : {(void *)c->zinv, (void *)c->gc, (void *)c->d_w}) if (q) hipFree(q);
    delete c;
}

int64_t shapemol_sd_tile(const shapemol_sd_ctx *c) { return c ? kSdTile : 0; }

int shapemol_sd_decode(shapemol_sd_ctx *c, const float *d_p, const int32_t *d_shape_of, int64_t n_points, int64_t points_per_shape,
                       const float *d_z, int64_t n_shapes, float *d_out, void *stream) {
    if (!c) return sd_fail("shapemol_sd_decode: null context");
    if (n_shapes < 1 || n_shapes > kMaxShapes) return sd_fail("shapemol_sd_decode: n_shapes must be in 1..65535, got " + std::to_string(n_shapes));
    if (n_points < 0 || n_points >= ((int64_t)1 << 31))
        return sd_fail("shapemol_sd_decode: n_points must be below 2^31 = 2147483648, got " + std::to_string(n_points));
    if (!d_shape_of && (points_per_shape < 0 || n_points != n_shapes * points_per_shape))
        return sd_fail("shapemol_sd_decode: without shape_of, n_points must be n_shapes * points_per_shape; got " + std::to_string(n_points) +
                       " points for " + std::to_string(n_shapes) + " x " + std::to_string(points_per_shape));
    if (n_points == 0) return 0;
    if (!d_p || !d_z || !d_out) return sd_fail("shapemol_sd_decode: null argument");
    SDCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (n_shapes > c->capB) {
        SDCHK(hipDeviceSynchronize());
        for (void *q : {(void *)c->zinv, (void *)c->gc}) if (q) hipFree(q);
        c->zinv = c->gc = nullptr; c->capB = 0;
        SDCHK(hipMalloc((void **)&c->zinv, (size_t)n_shapes * c->Z * 4));
        SDCHK(hipMalloc((void **)&c->gc, (size_t)n_shapes * kSdH * 4 * 4));
        c->capB = n_shapes;
    }
    c->lastB = n_shapes;
    const float *W = c->d_w;
    hipLaunchKernelGGL(sd_prologue_kernel, dim3((unsigned)n_shapes), dim3(256), 0, s, d_z, W + c->o_zin, W + c->o_win, W + c->o_bin, c->Z, c->zinv, c->gc);
    SdArgs a{};
    a.p = d_p; a.shape_of = d_shape_of; a.gc = c->gc; a.w0 = W + c->o_w0; a.img = W + c->o_img; a.bias = W + c->o_bias; a.w_out = W + c->o_out;
    a.out = d_out; a.n = n_points; a.per_shape = points_per_shape > 0 ? points_per_shape : 1; a.B = (int)n_shapes; a.L = c->L; a.sigmoid = c->sigmoid;
    // one workgroup per CU (its two weight images fill most of the CU's LDS), striding over the tiles
    const int64_t n_tiles = (n_points + kSdTile - 1) / kSdTile;
    const unsigned grid = (unsigned)(n_tiles < c->n_cu ? n_tiles : c->n_cu);
    hipLaunchKernelGGL(sd_decode_kernel, dim3(grid), dim3(kSdWaves * 64), c->lds_bytes, s, a);
    SDCHK(hipGetLastError());
    return 0;
}

int shapemol_sd_debug_read(shapemol_sd_ctx *c, int32_t what, void *h_dst, size_t n_bytes) {
    if (!c || !h_dst) return sd_fail("shapemol_sd_debug_read: null argument");
    if (c->lastB == 0) return sd_fail("shapemol_sd_debug_read: no shapemol_sd_decode has run on this context");
    const size_t B = (size_t)c->lastB, H = kSdH, Z = c->Z;
    if (what < SHAPEMOL_SD_ZINV || what > SHAPEMOL_SD_C)
        return sd_fail("shapemol_sd_debug_read: what must be SHAPEMOL_SD_ZINV, SHAPEMOL_SD_G or SHAPEMOL_SD_C (0 .. 2), got " + std::to_string(what));
    const size_t need = what == SHAPEMOL_SD_ZINV ? B * Z * 4 : what == SHAPEMOL_SD_G ? B * H * 3 * 4 : B * H * 4;
    if (n_bytes != need) return sd_fail("shapemol_sd_debug_read: buffer " + std::to_string(what) + " of the last decode has " + std::to_string(need) + " bytes, n_bytes is " + std::to_string(n_bytes));
    SDCHK(hipSetDevice(c->device));
    SDCHK(hipDeviceSynchronize());
    if (what == SHAPEMOL_SD_ZINV) { SDCHK(hipMemcpy(h_dst, c->zinv, need, hipMemcpyDeviceToHost)); return 0; }
    std::vector<float> gc(B * H * 4);
    SDCHK(hipMemcpy(gc.data(), c->gc, gc.size() * 4, hipMemcpyDeviceToHost));
    float *dst = (float *)h_dst;
    for (size_t e = 0; e < B * H; ++e) {
        if (what == SHAPEMOL_SD_G) for (int k = 0; k < 3; ++k) dst[e * 3 + k] = gc[e * 4 + k];
        else dst[e] = gc[e * 4 + 3];
    }
    return 0;
}

}  // extern "C"
