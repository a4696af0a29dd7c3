// Host side of the weights: the packed weight array (shapemol_amd/packing.py) -> the device image the kernels read
// (MFMA A-fragment images, split bf16 / f16 pieces, LDS images of the edge kernels).  Pure host arithmetic: no HIP API
// call, so the image can be built (and is tested) on a machine without a GPU.
#pragma once
#include "../../include/shapemol_hip.h"
#include "sm_edge.h"
#include "sm_edge_stream.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;      // shapemol_last_error()
int fail(const std::string &m) { g_err = m; return 1; }

// ---- host view of the packed weight array (order documented in shapemol_amd/packing.py) ----
struct Lin { const float *w = nullptr, *b = nullptr; int out = 0, in = 0; };
struct Mlp { Lin l1; const float *g = nullptr, *be = nullptr; Lin l2; };
struct Cursor {
    const float *p; size_t left;
    bool ok = true;
    const float *take(size_t n) {
        if (n > left) { ok = false; return p; }
        const float *r = p; p += n; left -= n; return r;
    }
    Lin lin(int out, int in, bool bias = true) {
        Lin l; l.out = out; l.in = in; l.w = take((size_t)out * in); l.b = bias ? take(out) : nullptr; return l;
    }
    Mlp mlp(int in, int hid, int out) {
        Mlp m; m.l1 = lin(hid, in); m.g = take(hid); m.be = take(hid); m.l2 = lin(out, hid); return m;
    }
};
struct HostLayer { Mlp hk, hv, hq, no, xk, xv, xq; const float *vn_f, *bn_g, *bn_b, *vn_d; };
struct HostModel {
    const float *tab[7];
    Lin te1, te2, emb;
    Mlp ew;
    std::vector<HostLayer> layer;
    Mlp inv;
    Lin v1, v2;
};

size_t weight_count(const shapemol_config &c) {
    const size_t H = c.hidden_dim, G = c.num_r_gaussian, S = c.shape_dim, SL = c.shape_latent_dim,
                 D = c.time_emb_dim, C = c.num_classes, T = c.num_timesteps, hd = c.n_heads;
    const size_t kv = G + 2 * H + SL, cin = 1 + hd + S;
    auto mlp = [](size_t in, size_t hid, size_t out) { return hid * in + hid + 2 * hid + out * hid + out; };
    size_t n = 7 * T;
    n += 2 * D * D + 2 * D + D * 2 * D + D;
    n += H * (C + D) + H;
    n += mlp(G, H, 1);
    const size_t per_layer = 2 * mlp(kv, H, H) + mlp(H, H, H) + mlp(2 * H, H, H) + mlp(kv, H, H) +
                             mlp(kv, H, hd) + mlp(H, H, H) + 2 * hd * cin + 2 * hd;
    n += (size_t)c.num_layers * per_layer;
    n += mlp(S, S, SL);
    n += H * H + H + C * H + C;
    return n;
}

bool parse_weights(const shapemol_config &c, const float *w, size_t n, HostModel &m) {
    const int H = c.hidden_dim, G = c.num_r_gaussian, S = c.shape_dim, SL = c.shape_latent_dim,
              D = c.time_emb_dim, C = c.num_classes, T = c.num_timesteps, hd = c.n_heads;
    const int kv = G + 2 * H + SL, cin = 1 + hd + S;
    Cursor cu{w, n};
    for (int i = 0; i < 7; ++i) m.tab[i] = cu.take(T);
    m.te1 = cu.lin(2 * D, D);
    m.te2 = cu.lin(D, 2 * D);
    m.emb = cu.lin(H, C + D);
    m.ew = cu.mlp(G, H, 1);
    m.layer.resize(c.num_layers);
    for (auto &L : m.layer) {
        L.hk = cu.mlp(kv, H, H); L.hv = cu.mlp(kv, H, H); L.hq = cu.mlp(H, H, H); L.no = cu.mlp(2 * H, H, H);
        L.xk = cu.mlp(kv, H, H); L.xv = cu.mlp(kv, H, hd); L.xq = cu.mlp(H, H, H);
        L.vn_f = cu.take((size_t)hd * cin); L.bn_g = cu.take(hd); L.bn_b = cu.take(hd); L.vn_d = cu.take((size_t)hd * cin);
    }
    m.inv = cu.mlp(S, S, SL);
    m.v1 = cu.lin(H, H);
    m.v2 = cu.lin(C, H);
    return cu.ok && cu.left == 0;
}

// ---- device image builder --------------------------------------------------------------------
struct Image {
    std::vector<float> d;
    size_t alloc(size_t n) {
        const size_t off = (d.size() + 63) & ~size_t(63);
        d.resize(off + n, 0.f);
        return off;
    }
    size_t put(const float *src, size_t n) { const size_t o = alloc(n); std::memcpy(&d[o], src, n * sizeof(float)); return o; }
};

struct DevMlp { size_t w1, b1, g, be, w2, b2; };            // raw row-major (VALU kernels)
struct DevMlpImg { size_t w1img, b1, g, be, w2img, b2; int nt2; size_t w1img6, w2img6, w1img16, w2img16; };   // MFMA A-fragment images (sm_node.h)
struct DevLayer {
    size_t pre_x2h, pre_h2x;          // images of [4H][H]: first-layer node blocks (k_i, k_j, v_i, v_j)
    size_t lin_img;                   // image of [8H][H]: pre_h2x of this layer followed by pre_x2h of the next
    size_t lin6_img, pre6_x2h;        // the same (and pre_x2h alone) as split bf16 images (node_linear6_kernel)
    size_t lin16_img, pre16_x2h;      // ... and as two-piece f16 images (node_linear16_kernel)
    size_t sk_x2h, sv_x2h, sk_h2x, sv_h2x;   // [H][SL] shape columns of the first layers
    size_t bk_x2h, bv_x2h, bk_h2x, bv_h2x;   // first-layer biases [H]
    DevMlpImg q_x2h, q_h2x, no;
    size_t blob_x2h, blob_h2x;        // fp32 edge kernels (sm_edge.h): both MLPs of a kernel in one LDS image
    size_t img_kx, img_vx, img_kh, img_vh;   // bf16-split phase kernels (sm_edge_bf16.h): one image per MLP
    size_t i16_kx, i16_vx, i16_kh, i16_vh;   // two-piece f16 images (sm_edge16.h)
    size_t st_kx, st_vx, st_kh, st_vh;       // streaming kernels (sm_edge_stream.h): producer parts (LDS images) ...
    size_t sw2_kx, sw2_vx, sw2_kh;           // ... and the second Linears as three bf16 pieces (consumers' registers)
    size_t sb2_vx;                           // bias of the x2h value MLP's second Linear [H]
    size_t vn_f, vn_d;                // original [heads][cin]
    size_t wf_x, wd_x, wf_o, wd_o, bn_g, bn_b;
};
struct DevModel {
    size_t tab[7];
    size_t te1w, te1b, te2w, te2b, embw, embb, embwT;
    DevMlp ew, inv;
    DevMlpImg vhead;             // Linear -> SSP -> Linear (second image padded to 16 rows)
    std::vector<DevLayer> layer;
};

// A-fragment image of W[rows][K] taken from src[r * ld + col0 + c]; rows padded with zeros to rows_pad
size_t pack_image(Image &im, const float *src, int rows, int rows_pad, int K, int ld, int col0) {
    const int ntk = K / 16;
    const size_t o = im.alloc((size_t)rows_pad * K);
    for (int t2 = 0; t2 < rows_pad / 16; ++t2)
        for (int t = 0; t < ntk; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t2 + (lane & 15), col = 16 * t + 4 * (lane >> 4) + r;
                    im.d[o + ((size_t)(t2 * ntk + t) * 64 + lane) * 4 + r] = row < rows ? src[(size_t)row * ld + col0 + col] : 0.f;
                }
    return o;
}
size_t put_padded(Image &im, const float *src, int n, int n_pad) {
    const size_t o = im.alloc(n_pad);
    std::memcpy(&im.d[o], src, n * sizeof(float));
    return o;
}
// exact 3-way bf16 split of a float by truncation; returns the three 16-bit patterns
void split3_host(float w, uint16_t (&p)[3]) {
    float r = w;
    for (int i = 0; i < 3; ++i) {
        uint32_t u; std::memcpy(&u, &r, 4);
        const uint32_t hi = u & 0xFFFF0000u;
        p[i] = (uint16_t)(hi >> 16);
        float h; std::memcpy(&h, &hi, 4);
        r = r - h;
    }
}

// hi + lo two-piece f16 split (both round-to-nearest): the 16-bit patterns
void split2_host(float w, uint16_t (&p)[2]) {
    const _Float16 h = (_Float16)w;
    const _Float16 l = (_Float16)(w - (float)h);
    std::memcpy(&p[0], &h, 2);
    std::memcpy(&p[1], &l, 2);
}

// The split operand images: word q of a lane holds its elements j = 2q (low half) and 2q + 1 (high half), each split into
// PIECES 16-bit pieces (3: exact bf16, split3_host; 2: f16 hi + lo, split2_host); piece p of the word goes to dst[at(p, lane, q)]
template <int PIECES, typename Elem, typename At>
void put_split_words(uint32_t *dst, int n_words, Elem elem, At at) {
    for (int lane = 0; lane < 64; ++lane)
        for (int q = 0; q < n_words; ++q) {
            uint16_t pc[2][PIECES];
            for (int e = 0; e < 2; ++e) {
                if constexpr (PIECES == 3) split3_host(elem(lane, 2 * q + e), pc[e]);
                else split2_host(elem(lane, 2 * q + e), pc[e]);
            }
            for (int p = 0; p < PIECES; ++p) dst[at(p, lane, q)] = (uint32_t)pc[0][p] | ((uint32_t)pc[1][p] << 16);
        }
}
// element j of a lane in feature tile t of an edge MLP's RBF block (first Linear, columns 0..19 of kv_in; j >= 5: padding)
float rbf_w(const Mlp &m, int kv_in, int t, int lane, int j) {
    return j < 5 ? m.l1.w[(size_t)(16 * t + (lane & 15)) * kv_in + 4 * j + (lane >> 4)] : 0.f;
}
// element j of a lane in K block b (32 columns) of row `row` of an edge MLP's second Linear [.][H] (row < 0: padding)
float w2_w(const Mlp &m, int H, int row, int b, int lane, int j) {
    return row < 0 ? 0.f : m.l2.w[(size_t)row * H + 16 * (2 * b + (j >> 2)) + 4 * (lane >> 4) + (j & 3)];
}

// fp32 A-fragment image of W[rows][K] (pack_image) -> its split image, element order of gemm_bf16x6:
//   [(((ot * PIECES + piece) * NB + b) * 64 + lane) * 4 + q] u32
// PIECES = 3: node_linear6_kernel / node_chain6_kernel; 2: node_linear16_kernel / node_chain16_kernel
template <int PIECES>
size_t pack_linear_split(Image &im, size_t src, int rows, int K) {
    const int ntk = K / 16, NB = K / 32, nto = rows / 16;
    const size_t o = im.alloc((size_t)nto * PIECES * NB * 256);
    uint32_t *w = reinterpret_cast<uint32_t *>(&im.d[o]);
    for (int ot = 0; ot < nto; ++ot)
        for (int b = 0; b < NB; ++b)
            put_split_words<PIECES>(w, 4, [&](int lane, int j) { return im.d[src + ((size_t)(ot * ntk + 2 * b + (j >> 2)) * 64 + lane) * 4 + (j & 3)]; },
                                    [&](int p, int lane, int q) { return (((size_t)(ot * PIECES + p) * NB + b) * 64 + lane) * 4 + q; });
    return o;
}

DevMlpImg put_mlp_img(Image &im, const Mlp &m) {
    DevMlpImg d;
    const int r2 = (m.l2.out + 15) / 16 * 16;
    d.w1img = pack_image(im, m.l1.w, m.l1.out, m.l1.out, m.l1.in, m.l1.in, 0);
    d.b1 = im.put(m.l1.b, m.l1.out);
    d.g = m.g ? im.put(m.g, m.l1.out) : 0; d.be = m.be ? im.put(m.be, m.l1.out) : 0;
    d.w2img = pack_image(im, m.l2.w, m.l2.out, r2, m.l2.in, m.l2.in, 0);
    d.b2 = put_padded(im, m.l2.b, m.l2.out, r2);
    d.nt2 = r2 / 16;
    d.w1img6 = pack_linear_split<3>(im, d.w1img, m.l1.out, m.l1.in);
    d.w2img6 = pack_linear_split<3>(im, d.w2img, r2, m.l2.in);
    d.w1img16 = pack_linear_split<2>(im, d.w1img, m.l1.out, m.l1.in);
    d.w2img16 = pack_linear_split<2>(im, d.w2img, r2, m.l2.in);
    return d;
}

int head_of_row(int m, int nt) {     // value row 4g + r of the h2x edge kernel -> head index, -1 = padding
    const int g = m >> 2, r = m & 3;
    if (r >= nt / 2) return -1;
    return 2 * ((nt / 2) * (g & 1) + r) + (g >> 1);
}
// row of the second Linear behind output row 16 * t2 + mrow of an LDS-resident edge MLP (the heads-wide value MLP of h2x
// keeps its heads in the order of head_of_row)
int w2_row(bool perm_heads, int NT, int t2, int mrow) { return perm_heads ? head_of_row(mrow, NT) : 16 * t2 + mrow; }

// LayerNorm gain and shift [H] and the second Linear's bias [nt2 * 16] of such an MLP
void put_ln_b2(const Mlp &m, int H, int nt2, bool perm_heads, float *gam, float *bet, float *b2) {
    std::memcpy(gam, m.g, H * sizeof(float));
    std::memcpy(bet, m.be, H * sizeof(float));
    for (int i = 0; i < nt2 * 16; ++i) {
        const int row = w2_row(perm_heads, H / 16, i / 16, i % 16);
        b2[i] = row < 0 ? 0.f : m.l2.b[row];
    }
}

// pack one edge MLP into the EdgeBlob image (see sm_edge.h)
void pack_edge_mlp(const Mlp &m, int H, int kv_in, bool perm_heads, float *wr, float *w2, float *gam, float *bet, float *b2) {
    const int NT = H / 16;
    const int nt2 = perm_heads ? 1 : NT;
    for (int t = 0; t < NT; ++t)
        for (int s = 0; s < 5; ++s)
            for (int lane = 0; lane < 64; ++lane) wr[(t * 5 + s) * 64 + lane] = rbf_w(m, kv_in, t, lane, s);
    for (int t2 = 0; t2 < nt2; ++t2)
        for (int t = 0; t < NT; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r)
                    w2[((t2 * NT + t) * 64 + lane) * 4 + r] = w2_w(m, H, w2_row(perm_heads, NT, t2, lane & 15), t / 2, lane, 4 * (t & 1) + r);
    put_ln_b2(m, H, nt2, perm_heads, gam, bet, b2);
}

// one edge MLP -> EdgePhaseImage (sm_edge_bf16.h)
template <int H>
size_t pack_phase_image(Image &im, const Mlp &m, int kv_in, bool perm_heads) {
    constexpr int NT = H / 16, NB = NT / 2;
    const int nt2 = perm_heads ? 1 : NT;
    const int G4 = (NT + 3) / 4;
    const bool bf1 = nt2 > 1;          // EdgePhaseImage::BF1
    const int o_wr = 0, o_g = o_wr + (bf1 ? 3 * NT * 256 : 5 * G4 * 256), o_b = o_g + H, o_b2 = o_b + H, o_w2 = o_b2 + nt2 * 16;
    const int total = o_w2 + 3 * nt2 * NB * 256;
    const size_t o = im.alloc(total);
    float *d = &im.d[o];
    uint32_t *wr = reinterpret_cast<uint32_t *>(d + o_wr), *w2 = reinterpret_cast<uint32_t *>(d + o_w2);
    for (int t = 0; t < NT; ++t) {
        if (bf1) put_split_words<3>(wr, 4, [&](int lane, int j) { return rbf_w(m, kv_in, t, lane, j); },
                                    [&](int p, int lane, int q) { return ((size_t)(p * NT + t) * 64 + lane) * 4 + q; });
        else for (int s = 0; s < 5; ++s)
            for (int lane = 0; lane < 64; ++lane) d[o_wr + ((s * G4 + t / 4) * 64 + lane) * 4 + (t & 3)] = rbf_w(m, kv_in, t, lane, s);
    }
    put_ln_b2(m, H, nt2, perm_heads, d + o_g, d + o_b, d + o_b2);
    for (int t2 = 0; t2 < nt2; ++t2)
        for (int b = 0; b < NB; ++b)
            put_split_words<3>(w2, 4, [&](int lane, int j) { return w2_w(m, H, w2_row(perm_heads, NT, t2, lane & 15), b, lane, j); },
                               [&](int p, int lane, int q) { return (((size_t)(p * nt2 + t2) * NB + b) * 64 + lane) * 4 + q; });
    return o;
}

// one edge MLP -> EdgeImage16 (sm_edge16.h); returns the largest |hidden activation| the LayerNorm of this MLP can
// produce (the fp16 range check of the caller)
template <int H>
float pack_image16(Image &im, const Mlp &m, int kv_in, bool perm_heads, size_t &img) {
    constexpr int NT = H / 16, NB = NT / 2;
    const int nt2 = perm_heads ? 1 : NT;
    const int o_w1 = 0, o_w2 = 2 * NT * 192, o_g = o_w2 + 2 * nt2 * NB * 256, o_b = o_g + H, o_b2 = o_b + H;
    const int total = (o_b2 + nt2 * 16 + 255) / 256 * 256;
    img = im.alloc(total);
    uint32_t *d = reinterpret_cast<uint32_t *>(&im.d[img]);
    for (int t = 0; t < NT; ++t)
        put_split_words<2>(d + o_w1, 3, [&](int lane, int j) { return rbf_w(m, kv_in, t, lane, j); },
                           [&](int p, int lane, int q) { return ((size_t)(p * NT + t) * 3 + q) * 64 + lane; });
    for (int t2 = 0; t2 < nt2; ++t2)
        for (int b = 0; b < NB; ++b)
            put_split_words<2>(d + o_w2, 4, [&](int lane, int j) { return w2_w(m, H, w2_row(perm_heads, NT, t2, lane & 15), b, lane, j); },
                               [&](int p, int lane, int q) { return (((size_t)(p * nt2 + t2) * NB + b) * 64 + lane) * 4 + q; });
    float *pp = &im.d[img];
    put_ln_b2(m, H, nt2, perm_heads, pp + o_g, pp + o_b, pp + o_b2);
    float gmax = 0.f, bmax = 0.f;
    for (int i = 0; i < H; ++i) { gmax = std::max(gmax, std::fabs(m.g[i])); bmax = std::max(bmax, std::fabs(m.be[i])); }
    return gmax * std::sqrt((float)(H - 1)) + bmax;
}

// one edge MLP -> the producer part of the streaming kernels (StreamMap<H, .>::P_*, sm_edge_stream.h): RBF block of the first
// Linear as three bf16 pieces (whole A fragments of the K = 32 step: centres 0..5 of lane group g in words 0..2, word 3 zero), gamma, beta, b2 and,
// for the heads-wide value MLP of h2x, the second Linear (rows = heads in natural order, padded to 16)
template <int H>
size_t pack_stream_part(Image &im, const Mlp &m, int kv_in, bool h2x_value) {
    constexpr int NT = H / 16, NB = NT / 2;
    using MX = StreamMap<H, false>; using MH = StreamMap<H, true>;
    const int total = h2x_value ? MH::PART_V : MX::PART_K;
    const size_t o = im.alloc(total);
    uint32_t *d = reinterpret_cast<uint32_t *>(&im.d[o]);
    std::memset(d, 0, (size_t)total * 4);
    for (int t = 0; t < NT; ++t)
        put_split_words<3>(d + MX::P_W1, 3, [&](int lane, int j) { return rbf_w(m, kv_in, t, lane, j); },
                           [&](int p, int lane, int q) { return ((size_t)(p * NT + t) * 64 + lane) * 4 + q; });      // (word 3 stays zero)
    float *pp = &im.d[o];
    std::memcpy(pp + MX::P_G, m.g, H * sizeof(float));
    std::memcpy(pp + MX::P_B, m.be, H * sizeof(float));
    std::memcpy(pp + MX::P_B2, m.l2.b, std::min(m.l2.out, H) * sizeof(float));
    for (int b = 0; h2x_value && b < NB; ++b)
        put_split_words<3>(d + MH::P_W2, 4, [&](int lane, int j) { return w2_w(m, H, (lane & 15) < m.l2.out ? (lane & 15) : -1, b, lane, j); },
                           [&](int p, int lane, int q) { return (((size_t)p * NB + b) * 64 + lane) * 4 + q; });
    return o;
}

// second Linear [H][H] of an edge MLP as three bf16 pieces [3][NT][NB][64][4] u32, element order of gemm_bf16x6 (rows natural)
template <int H>
size_t pack_stream_w2(Image &im, const Mlp &m) {
    constexpr int NT = H / 16, NB = NT / 2;
    const size_t o = im.alloc((size_t)3 * NT * NB * 256);
    uint32_t *w2 = reinterpret_cast<uint32_t *>(&im.d[o]);
    for (int t2 = 0; t2 < NT; ++t2)
        for (int b = 0; b < NB; ++b)
            put_split_words<3>(w2, 4, [&](int lane, int j) { return w2_w(m, H, 16 * t2 + (lane & 15), b, lane, j); },
                               [&](int p, int lane, int q) { return (((size_t)(p * NT + t2) * NB + b) * 64 + lane) * 4 + q; });
    return o;
}

template <int H>
int build_layer_image(const shapemol_config &c, const HostLayer &L, Image &im, DevLayer &D, float &hid_max) {
    const int G = c.num_r_gaussian, SL = c.shape_latent_dim, S = c.shape_dim, hd = c.n_heads;
    const int kv = G + 2 * H + SL, cin = 1 + hd + S, NT = H / 16;
    bool contiguous = true;
    auto put_pre = [&](const Mlp &k, const Mlp &v) {      // 4 images of [H][H]: k_i, k_j, v_i, v_j column blocks
        const Mlp *src[4] = {&k, &k, &v, &v};
        size_t first = 0;
        for (int blk = 0; blk < 4; ++blk) {
            const size_t o = pack_image(im, src[blk]->l1.w, H, H, H, kv, G + (blk & 1) * H);
            if (blk == 0) first = o;
            else if (o != first + (size_t)blk * H * H) contiguous = false;     // images must be contiguous
        }
        return first;
    };
    auto put_scols = [&](const Mlp &m) {
        const size_t o = im.alloc((size_t)H * SL);
        for (int f = 0; f < H; ++f) std::memcpy(&im.d[o + (size_t)f * SL], m.l1.w + (size_t)f * kv + G + 2 * H, SL * sizeof(float));
        return o;
    };
    D.pre_x2h = put_pre(L.hk, L.hv); D.pre_h2x = put_pre(L.xk, L.xv);
    if (!contiguous) return fail("shapemol_create: packed first-layer images are not contiguous (H * H must be a multiple of 64)");
    D.sk_x2h = put_scols(L.hk); D.sv_x2h = put_scols(L.hv); D.sk_h2x = put_scols(L.xk); D.sv_h2x = put_scols(L.xv);
    D.bk_x2h = im.put(L.hk.l1.b, H); D.bv_x2h = im.put(L.hv.l1.b, H);
    D.bk_h2x = im.put(L.xk.l1.b, H); D.bv_h2x = im.put(L.xv.l1.b, H);
    D.q_x2h = put_mlp_img(im, L.hq); D.q_h2x = put_mlp_img(im, L.xq); D.no = put_mlp_img(im, L.no);
    {
        using B = EdgeBlob<H, false>;
        const size_t o = im.alloc(B::TOTAL); D.blob_x2h = o; float *b = &im.d[o];
        pack_edge_mlp(L.hk, H, kv, false, b + B::K_WR, b + B::K_W2, b + B::K_G, b + B::K_B, b + B::K_B2);
        pack_edge_mlp(L.hv, H, kv, false, b + B::V_WR, b + B::V_W2, b + B::V_G, b + B::V_B, b + B::V_B2);
    }
    {
        using B = EdgeBlob<H, true>;
        const size_t o = im.alloc(B::TOTAL); D.blob_h2x = o; float *b = &im.d[o];
        pack_edge_mlp(L.xk, H, kv, false, b + B::K_WR, b + B::K_W2, b + B::K_G, b + B::K_B, b + B::K_B2);
        pack_edge_mlp(L.xv, H, kv, true, b + B::V_WR, b + B::V_W2, b + B::V_G, b + B::V_B, b + B::V_B2);
    }
    D.img_kx = pack_phase_image<H>(im, L.hk, kv, false); D.img_vx = pack_phase_image<H>(im, L.hv, kv, false);
    D.img_kh = pack_phase_image<H>(im, L.xk, kv, false); D.img_vh = pack_phase_image<H>(im, L.xv, kv, true);
    hid_max = std::max(hid_max, pack_image16<H>(im, L.hk, kv, false, D.i16_kx));
    hid_max = std::max(hid_max, pack_image16<H>(im, L.hv, kv, false, D.i16_vx));
    hid_max = std::max(hid_max, pack_image16<H>(im, L.xk, kv, false, D.i16_kh));
    hid_max = std::max(hid_max, pack_image16<H>(im, L.xv, kv, true, D.i16_vh));
    D.st_kx = pack_stream_part<H>(im, L.hk, kv, false); D.st_vx = pack_stream_part<H>(im, L.hv, kv, false);
    D.st_kh = pack_stream_part<H>(im, L.xk, kv, false); D.st_vh = pack_stream_part<H>(im, L.xv, kv, true);
    D.sw2_kx = pack_stream_w2<H>(im, L.hk); D.sw2_vx = pack_stream_w2<H>(im, L.hv); D.sw2_kh = pack_stream_w2<H>(im, L.xk);
    D.sb2_vx = im.put(L.hv.l2.b, H);
    D.vn_f = im.put(L.vn_f, (size_t)hd * cin); D.vn_d = im.put(L.vn_d, (size_t)hd * cin);
    D.bn_g = im.put(L.bn_g, hd); D.bn_b = im.put(L.bn_b, hd);
    D.wf_x = im.alloc(hd); D.wd_x = im.alloc(hd); D.wf_o = im.alloc((size_t)hd * 16); D.wd_o = im.alloc((size_t)hd * 16);
    for (int ch = 0; ch < hd; ++ch) {
        im.d[D.wf_x + ch] = L.vn_f[(size_t)ch * cin];
        im.d[D.wd_x + ch] = L.vn_d[(size_t)ch * cin];
        for (int m = 0; m < 16; ++m) {
            const int hh = head_of_row(m, NT);
            im.d[D.wf_o + ch * 16 + m] = hh < 0 ? 0.f : L.vn_f[(size_t)ch * cin + 1 + hh];
            im.d[D.wd_o + ch * 16 + m] = hh < 0 ? 0.f : L.vn_d[(size_t)ch * cin + 1 + hh];
        }
    }
    return 0;
}

// the whole device image of a model: offsets into im.d in dm, fp16 range bound of the edge MLPs' hidden activations in hid_max
int build_model_image(const shapemol_config &cfg, const HostModel &hm, Image &im, DevModel &dm, float &hid_max) {
    const int H = cfg.hidden_dim, T = cfg.num_timesteps;
    for (int i = 0; i < 7; ++i) dm.tab[i] = im.put(hm.tab[i], T);
    dm.te1w = im.put(hm.te1.w, (size_t)hm.te1.out * hm.te1.in); dm.te1b = im.put(hm.te1.b, hm.te1.out);
    dm.te2w = im.put(hm.te2.w, (size_t)hm.te2.out * hm.te2.in); dm.te2b = im.put(hm.te2.b, hm.te2.out);
    dm.embw = im.put(hm.emb.w, (size_t)hm.emb.out * hm.emb.in); dm.embb = im.put(hm.emb.b, hm.emb.out);
    dm.embwT = im.alloc((size_t)hm.emb.in * hm.emb.out);          // [C + D][H]
    for (int f = 0; f < hm.emb.out; ++f)
        for (int k = 0; k < hm.emb.in; ++k) im.d[dm.embwT + (size_t)k * hm.emb.out + f] = hm.emb.w[(size_t)f * hm.emb.in + k];
    auto put_mlp = [&](const Mlp &m) {
        DevMlp d;
        d.w1 = im.put(m.l1.w, (size_t)m.l1.out * m.l1.in); d.b1 = im.put(m.l1.b, m.l1.out);
        d.g = im.put(m.g, m.l1.out); d.be = im.put(m.be, m.l1.out);
        d.w2 = im.put(m.l2.w, (size_t)m.l2.out * m.l2.in); d.b2 = im.put(m.l2.b, m.l2.out);
        return d;
    };
    dm.ew = put_mlp(hm.ew);
    dm.inv = put_mlp(hm.inv);
    {
        Mlp vh; vh.l1 = hm.v1; vh.l2 = hm.v2; vh.g = nullptr; vh.be = nullptr;
        dm.vhead = put_mlp_img(im, vh);
    }
    dm.layer.resize(cfg.num_layers);
    for (int l = 0; l < cfg.num_layers; ++l) {
        if (H == 128 ? build_layer_image<128>(cfg, hm.layer[l], im, dm.layer[l], hid_max)
                     : build_layer_image<32>(cfg, hm.layer[l], im, dm.layer[l], hid_max)) return 1;
    }
    for (int l = 0; l < cfg.num_layers; ++l) {      // paired images: pre_h2x(l) | pre_x2h(l + 1)
        const size_t blk = (size_t)4 * H * H;
        const size_t o = im.alloc(2 * blk);
        std::memcpy(&im.d[o], &im.d[dm.layer[l].pre_h2x], blk * sizeof(float));
        if (l + 1 < cfg.num_layers) std::memcpy(&im.d[o + blk], &im.d[dm.layer[l + 1].pre_x2h], blk * sizeof(float));
        dm.layer[l].lin_img = o;
    }
    for (int l = 0; l < cfg.num_layers; ++l) {
        dm.layer[l].lin6_img = pack_linear_split<3>(im, dm.layer[l].lin_img, 8 * H, H);
        dm.layer[l].pre6_x2h = l == 0 ? pack_linear_split<3>(im, dm.layer[l].pre_x2h, 4 * H, H) : 0;
        dm.layer[l].lin16_img = pack_linear_split<2>(im, dm.layer[l].lin_img, 8 * H, H);
        dm.layer[l].pre16_x2h = l == 0 ? pack_linear_split<2>(im, dm.layer[l].pre_x2h, 4 * H, H) : 0;
    }
    im.alloc(64);
    return 0;
}

}  // namespace
