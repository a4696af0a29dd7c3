// Training the shape encoder: the training variant of the forward (deterministic batch statistics) and the backward of
// VN_DGCNN_Encoder with respect to every parameter.  No gradient flows to the points or through the
// neighbour lists.  Nothing here uses a floating-point atomic: every sum that crosses threads is taken in a fixed order, in
// float64 where partials meet, so the latent and every gradient are bit-identical from run to run.
//
// Forward.  The sweep of sm_shape.h (se_forward of shape_encoder.hip issues it for both paths), except the two kernels that add the
// batch sums with atomics: se_*_stats_part_kernel leaves one float64 partial per workgroup (a fixed number of workgroups, each
// walking its points in order, a point's sums by the device function the atomic kernels use) and se_stats_reduce_kernel adds them in
// workgroup order.  It writes the totals into replica 0 of the accumulator the apply kernels read (the other replicas zero), so
// se_edge_apply_kernel / se_head_apply_kernel run unchanged, and the batch mean and variance (se_mean_var, as the apply kernels
// take them) into the caller's buffer.
//
// Backward of a VN stage (edge e = (i, j), channel c; M = edges of the batch):
//     r = |p|, n = r + 1e-6, xh = (n - mean) / sig, s = gamma xh + beta, q = p s / n, dot = q.d, D = d.d + 1e-6,
//     o = q (dot >= 0) or q - 0.8 (dot / D) d;           upstream g_o
//     dot >= 0: g_q = g_o, g_d = 0;  else a = g_o.d, g_q = g_o - 0.8 (a / D) d,
//                                         g_d = -0.8 [(a / D) q + (dot / D) g_o - 2 (a dot / D^2) d]
//     g_s = (g_q.p) / n;   S1 = sum_e g_s (= dbeta),  S2 = sum_e g_s xh (= dgamma)
//     g_n = (gamma / sig) (g_s - S1 / M - xh S2 / M) - (g_q.p) s / n^2;    g_p = g_q s / n + g_n p / r   (p / r := 0 at r = 0)
// A block's p = Yf1[j] + Yf2[i], d = Yd1[j] + Yd2[i] with Y = W' h: dY[j][0:C] += g_p, dY[i][C:2C] += g_p, dY[j][2C:3C] += g_d,
// dY[i][3C:4C] += g_d.  The two j sums go through a reverse neighbour list (CSR by j in edge order, built by a scan: se_deg_kernel,
// se_rowptr_kernel, se_rev_fill_kernel); se_edge_bwd_gather_kernel gives every (point, channel) one thread that recomputes its 20
// outgoing and its incoming edges and writes its four dY rows once.  Then the two products on the fp32 matrix cores:
// se_dhin_kernel dh_in = W'^T dY and se_dw_kernel dW' = sum over (point, xyz) of dY h^T (split over the points, partials added in
// split order in float64 by se_dw_finish_kernel, which also maps dW' back to map_to_feat / map_to_dir).
#pragma once
#include "sm_shape.h"

constexpr int kSeParts = 256;       // workgroups of a fixed-order sum (each leaves one partial per channel)
constexpr int kSePartQ = 6;         // sums per channel a partial holds at most
constexpr int kSeCh = 256;          // channel stride of partials, sums and statistics (C = 128, latent_dim <= 256)
constexpr int kSeDwLd = 128 + 16;   // LDS row of se_dw_kernel (the four columns a k-step reads lie 16 banks apart)
constexpr int kSeDwMaxSplits = 64;

// ---- forward: deterministic batch statistics -----------------------------------------------------------------------------
// part [gridDim.x][kSePartQ][kSeCh]: sums of ||p|| + EPS and of its square over the workgroup's edges, edge order
template <bool L0>
__global__ void se_edge_stats_part_kernel(SeEdgeArgs a, double *part) {
    const int c = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int i = blockIdx.x; i < a.n_total; i += gridDim.x) se_edge_norm_sums<L0>(a, i, c, s1, s2);
    double *dst = part + (size_t)blockIdx.x * kSePartQ * kSeCh;
    dst[c] = s1; dst[kSeCh + c] = s2;
}
// the same over the points of conv_c's products pd [P][LAT + 1][3]; threads m < LAT
__global__ void se_head_stats_part_kernel(const float *pd, int n_total, int LAT, double *part) {
    const int m = threadIdx.x;
    if (m >= LAT) return;
    double s1 = 0.0, s2 = 0.0;
    for (int pt = blockIdx.x; pt < n_total; pt += gridDim.x) se_norm_sums(pd + ((size_t)pt * (LAT + 1) + m) * 3, s1, s2);
    double *dst = part + (size_t)blockIdx.x * kSePartQ * kSeCh;
    dst[m] = s1; dst[kSeCh + m] = s2;
}
// one workgroup, thread c < nch: totals into replica 0 of acc [kSeReplicas][2][nch], mean and biased variance (se_mean_var, the
// function the apply kernels take theirs from) into stats [2][kSeCh]
__global__ void se_stats_reduce_kernel(const double *part, int n_parts, int nch, double cnt, double *acc, double *stats) {
    const int c = threadIdx.x;
    if (c >= nch) return;
    double t1 = 0.0, t2 = 0.0;
    for (int b = 0; b < n_parts; ++b) { t1 += part[(size_t)b * kSePartQ * kSeCh + c]; t2 += part[(size_t)b * kSePartQ * kSeCh + kSeCh + c]; }
    acc[c] = t1; acc[nch + c] = t2;
    for (int r = 1; r < kSeReplicas; ++r) { acc[(size_t)r * 2 * nch + c] = 0.0; acc[(size_t)r * 2 * nch + nch + c] = 0.0; }
    double mean, var;
    se_mean_var(t1, t2, cnt, mean, var);
    stats[c] = mean; stats[kSeCh + c] = var;
}

// ---- the gradient of one VN batch-norm + leaky-ReLU element -------------------------------------------------------------------
struct SeVnGrad { float gs, xh, gp[3], gd[3]; bool neg; };
// m1 = S1 / M, m2 = S2 / M (0 in the pass that takes S1 and S2: only gs and xh are used there)
SM_DEV SeVnGrad se_vn_grad(const float (&p)[3], const float (&d)[3], float mean, float rstd, float g, float b, const float (&go)[3], float m1, float m2) {
    SeVnGrad o;
    const float r = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]), n = r + 1e-6f;
    const float xh = (n - mean) * rstd, s = xh * g + b;
    float q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = p[k] / n * s;
    const float dot = q[0] * d[0] + q[1] * d[1] + q[2] * d[2];
    const float D = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + 1e-6f;
    float gq[3];
    o.neg = !(dot >= 0.f);
    if (dot >= 0.f) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { gq[k] = go[k]; o.gd[k] = 0.f; }
    } else {
        const float a = go[0] * d[0] + go[1] * d[1] + go[2] * d[2];
        const float aD = a / D, dD = dot / D, add = 2.f * (a * dot / (D * D));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gq[k] = go[k] - 0.8f * aD * d[k];
            o.gd[k] = -0.8f * (aD * q[k] + dD * go[k] - add * d[k]);
        }
    }
    const float t = gq[0] * p[0] + gq[1] * p[1] + gq[2] * p[2];
    o.gs = t / n; o.xh = xh;
    const float gn = g * rstd * (o.gs - m1 - xh * m2) - t * s / (n * n);
    const float sn = s / n, gr = r > 0.f ? gn / r : 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.gp[k] = gq[k] * sn + gr * p[k];
    return o;
}

struct SeBwdArgs {
    SeEdgeArgs e;            // the stage's forward operands (y, x, w0f, w0d, idx, bn_g, bn_b, n_total, N, C)
    const double *stats;     // [2][kSeCh] batch mean and variance of the stage (saved by the forward)
    const float *dH;         // gradient of the stage's output: dH[i * dh_ld + dh_off + c * 3 + xyz]
    int dh_ld, dh_off;
    const double *S;         // [kSePartQ][kSeCh]: S1, S2 of the stage
    const int *deg, *rowptr, *rev;
    float *dY;               // [P][4 C][3]
    int *mask;               // null, or [P][kSeCh]: bit kk of [i][c] = edge (i, kk) of channel c took the branch dot < 0 (diagnostic)
};

// neighbour of entry e of the lists, as a point of the batch.  An entry outside [0, N) cannot come from se_knn_kernel; it is clamped
// so that no list, whatever it holds, leads outside the buffers
SM_DEV int se_nbr(const int *idx, size_t e, int base, int N) { return base + (int)min((unsigned)idx[e], (unsigned)(N - 1)); }

SM_DEV void se_stage_consts(const SeBwdArgs &a, int c, double M, float &mean, float &rstd, float &m1, float &m2) {
    mean = (float)a.stats[c];
    rstd = 1.0f / sqrtf((float)a.stats[kSeCh + c] + 1e-5f);
    m1 = a.S ? (float)(a.S[c] / M) : 0.f;
    m2 = a.S ? (float)(a.S[kSeCh + c] / M) : 0.f;
}

// PASS 0: S1, S2.  PASS 1 (conv_pos only, S given): the four weight-gradient vectors g_p.(x_j - x_i), g_p.x_i, g_d.(x_j - x_i), g_d.x_i
template <bool L0, int PASS>
__global__ void se_edge_bwd_sums_kernel(SeBwdArgs a, double *part) {
    const int c = threadIdx.x;
    float mean, rstd, m1, m2;
    se_stage_consts(a, c, (double)a.e.n_total * kSeK, mean, rstd, m1, m2);
    const float g = a.e.bn_g[c], b = a.e.bn_b[c];
    double s[PASS == 0 ? 2 : 4] = {};
    for (int i = blockIdx.x; i < a.e.n_total; i += gridDim.x) {
        const int base = (i / a.e.N) * a.e.N;
        const float *dh = a.dH + (size_t)i * a.dh_ld + a.dh_off + c * 3;
        const float go[3] = {dh[0] / kSeK, dh[1] / kSeK, dh[2] / kSeK};
        unsigned bits = 0;
        for (int kk = 0; kk < kSeK; ++kk) {
            const int j = se_nbr(a.e.idx, (size_t)i * kSeK + kk, base, a.e.N);
            float p[3], d[3];
            se_edge_pd<L0>(a.e, i, j, c, p, d);
            const SeVnGrad v = se_vn_grad(p, d, mean, rstd, g, b, go, m1, m2);
            if constexpr (PASS == 0) { s[0] += (double)v.gs; s[1] += (double)v.gs * (double)v.xh; }
            else {
                bits |= (unsigned)v.neg << kk;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float xi = a.e.x[(size_t)i * 3 + k], dx = a.e.x[(size_t)j * 3 + k] - xi;
                    s[0] += (double)v.gp[k] * dx; s[1] += (double)v.gp[k] * xi; s[2] += (double)v.gd[k] * dx; s[3] += (double)v.gd[k] * xi;
                }
            }
        }
        if (PASS == 1 && a.mask) a.mask[(size_t)i * kSeCh + c] = (int)bits;
    }
    double *dst = part + (size_t)blockIdx.x * kSePartQ * kSeCh;
#pragma unroll
    for (int q = 0; q < (PASS == 0 ? 2 : 4); ++q) dst[q * kSeCh + c] = s[q];
}

// partials -> sums [nq][kSeCh] in workgroup order, and as float32 into up to kSePartQ destinations (dst[q][c * stride[q]])
struct SeSumDst { float *dst[kSePartQ]; int stride[kSePartQ]; };
__global__ void se_part_reduce_kernel(const double *part, int n_parts, int nq, int nch, double *sums, SeSumDst o) {
    const int c = threadIdx.x, q = blockIdx.x;
    if (c >= nch || q >= nq) return;
    double t = 0.0;
    for (int b = 0; b < n_parts; ++b) t += part[((size_t)b * kSePartQ + q) * kSeCh + c];
    sums[q * kSeCh + c] = t;
    if (o.dst[q]) o.dst[q][(size_t)c * o.stride[q]] = (float)t;
}

// ---- the reverse neighbour list --------------------------------------------------------------------------------------------
__global__ void se_deg_kernel(const int *idx, int n_total, int N, int *deg) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)n_total * kSeK) return;
    const int i = (int)(e / kSeK);
    atomicAdd(deg + se_nbr(idx, (size_t)e, (i / N) * N, N), 1);        // (integers: the counts do not depend on the order)
}
// one workgroup per shape: rowptr[b N + j] = b N k + (edges of the shape that end in a point before j)
__global__ void __launch_bounds__(256) se_rowptr_kernel(const int *deg, int N, int *rowptr) {
    __shared__ int sums[256];
    const int b = blockIdx.x, t = threadIdx.x, per = (N + 255) / 256;
    const int j0 = min(t * per, N), j1 = min(j0 + per, N);
    int s = 0;
    for (int j = j0; j < j1; ++j) s += deg[(size_t)b * N + j];
    sums[t] = s;
    __syncthreads();
    int off = b * N * kSeK;
    for (int k = 0; k < t; ++k) off += sums[k];
    for (int j = j0; j < j1; ++j) { rowptr[(size_t)b * N + j] = off; off += deg[(size_t)b * N + j]; }
}
// grid (N / 16, B), one wave per end point j (4 each): the shape's edges in edge order, those that end in j compacted with a ballot:
// rev[rowptr[j] ..] = their start points, ascending
__global__ void __launch_bounds__(256) se_rev_fill_kernel(const int *idx, int N, const int *rowptr, int *rev) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int *ib = idx + (size_t)b * N * kSeK;
    const int tot = N * kSeK;
    for (int jj = wave; jj < 16; jj += 4) {
        const int j = blockIdx.x * 16 + jj;
        if (j >= N) continue;
        const int start = rowptr[(size_t)b * N + j];
        int cnt = 0;
        for (int e0 = 0; e0 < tot; e0 += 64) {
            const int e = e0 + lane;
            const bool hit = e < tot && (int)min((unsigned)ib[e], (unsigned)(N - 1)) == j;
            const unsigned long long mask = __ballot(hit);
            if (hit) rev[start + cnt + __popcll(mask & ((1ull << lane) - 1ull))] = b * N + e / kSeK;
            cnt += __popcll(mask);
        }
    }
}

// ---- a block's dY: one workgroup of C threads per point -----------------------------------------------------------------------
__global__ void se_edge_bwd_gather_kernel(SeBwdArgs a) {
    const int x = blockIdx.x, c = threadIdx.x, C = a.e.C;
    const int base = (x / a.e.N) * a.e.N;
    float mean, rstd, m1, m2;
    se_stage_consts(a, c, (double)a.e.n_total * kSeK, mean, rstd, m1, m2);
    const float g = a.e.bn_g[c], b = a.e.bn_b[c];
    float ip[3] = {0.f, 0.f, 0.f}, id[3] = {0.f, 0.f, 0.f}, jp[3] = {0.f, 0.f, 0.f}, jd[3] = {0.f, 0.f, 0.f};
    {   // the point's own 20 edges (it is their i)
        const float *dh = a.dH + (size_t)x * a.dh_ld + a.dh_off + c * 3;
        const float go[3] = {dh[0] / kSeK, dh[1] / kSeK, dh[2] / kSeK};
        unsigned bits = 0;
        for (int kk = 0; kk < kSeK; ++kk) {
            const int j = se_nbr(a.e.idx, (size_t)x * kSeK + kk, base, a.e.N);
            float p[3], d[3];
            se_edge_pd<false>(a.e, x, j, c, p, d);
            const SeVnGrad v = se_vn_grad(p, d, mean, rstd, g, b, go, m1, m2);
            bits |= (unsigned)v.neg << kk;
#pragma unroll
            for (int k = 0; k < 3; ++k) { ip[k] += v.gp[k]; id[k] += v.gd[k]; }
        }
        if (a.mask) a.mask[(size_t)x * kSeCh + c] = (int)bits;
    }
    const int t0 = a.rowptr[x], t1 = t0 + a.deg[x];
    for (int t = t0; t < t1; ++t) {      // the edges that end in the point (it is their j), by ascending start point
        const int i = a.rev[t];
        const float *dh = a.dH + (size_t)i * a.dh_ld + a.dh_off + c * 3;
        const float go[3] = {dh[0] / kSeK, dh[1] / kSeK, dh[2] / kSeK};
        float p[3], d[3];
        se_edge_pd<false>(a.e, i, x, c, p, d);
        const SeVnGrad v = se_vn_grad(p, d, mean, rstd, g, b, go, m1, m2);
#pragma unroll
        for (int k = 0; k < 3; ++k) { jp[k] += v.gp[k]; jd[k] += v.gd[k]; }
    }
    float *o = a.dY + ((size_t)x * 4 * C + c) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = jp[k]; o[C * 3 + k] = ip[k]; o[2 * C * 3 + k] = jd[k]; o[3 * C * 3 + k] = id[k]; }
}

// ---- dh_in = W'^T dY on the fp32 matrix cores ---------------------------------------------------------------------------------
// wT: A fragments of W'^T (C rows, K = 4 C), in the layout of se_point_linear_kernel's wimg; from the forward image by a permutation
template <int C>
__global__ void se_wimg_transpose_kernel(const float *wimg, float *wT) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 4 * C * C) return;
    const int r = e & 3, lane = (e >> 2) & 63, ts = e >> 8, s4 = ts % (4 * C / 16), t = ts / (4 * C / 16);
    const int k = 16 * t + (lane & 15), m = 4 * (4 * s4 + r) + (lane >> 4);              // wT holds W'[m][k]
    wT[e] = wimg[((size_t)((m / 16) * (C / 16) + k / 16) * 64 + (k & 3) * 16 + (m & 15)) * 4 + ((k >> 2) & 3)];
}
// One workgroup (4 waves) per 16 columns (column = (point, component)); out[p * ld_out + off_out + row * 3 + xyz] (+)= the product
template <int C>
__global__ void __launch_bounds__(256) se_dhin_kernel(const float *dY, const float *wT, int n_cols, float *out, int ld_out, int off_out, int accumulate) {
    constexpr int K = 4 * C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int col = min(blockIdx.x * 16 + n, n_cols - 1);
    const int p = col / 3, c3 = col % 3;
    float x[K / 4];
#pragma unroll
    for (int s = 0; s < K / 4; ++s) x[s] = dY[(size_t)p * K * 3 + (4 * s + g) * 3 + c3];
    for (int t = wave; t < C / 16; t += 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s4 = 0; s4 < K / 16; ++s4) {
            const float4 a = ldg4(wT + ((size_t)(t * (K / 16) + s4) * 64 + lane) * 4);
            acc = mfma16(a.x, x[4 * s4 + 0], acc); acc = mfma16(a.y, x[4 * s4 + 1], acc);
            acc = mfma16(a.z, x[4 * s4 + 2], acc); acc = mfma16(a.w, x[4 * s4 + 3], acc);
        }
        if (blockIdx.x * 16 + n < n_cols) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float *o = out + (size_t)p * ld_out + off_out + (16 * t + 4 * g + r) * 3 + c3;
                *o = accumulate ? *o + acc[r] : acc[r];
            }
        }
    }
}

// ---- dW' = sum over (point, xyz) of dY h^T, split over groups of 16 points ------------------------------------------------------
// grid (4, splits): row block rb (128 rows of dY: Yf1 | Yf2 | Yd1 | Yd2) and a range of groups.  A group's 48 columns (16 points x
// xyz) of both operands go through LDS as [column][row]; the matrix cores take dY as the A operand (lane = row, k = column) and h as
// the B operand.  Wave w owns output rows 32 w .. 32 w + 31 and all eight column tiles.  pw [4][splits][128 * 128].
__global__ void __launch_bounds__(256) se_dw_kernel(const float *dY, const float *h, int ld_h, int n_groups, int per_split, float *pw) {
    constexpr int C = 128, ROW = C * 3;                   // floats of a point's row block, and of its features
    __shared__ __attribute__((aligned(16))) float ds[48 * kSeDwLd], as[48 * kSeDwLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int rb = blockIdx.x, split = blockIdx.y, splits = gridDim.y;
    const int g0 = split * per_split, g1 = min(g0 + per_split, n_groups);
    f32x4 acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // float4 f of a group (f = tid + 256 u, u < 6): point f / 96, floats 4 (f % 96) .. + 3 of its 384
    float4 rd[6], ra[6];
    auto fetch = [&](int grp) {
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            const int f = tid + 256 * u, pl = f / 96, q4 = f % 96;
            const size_t pt = (size_t)grp * 16 + pl;
            rd[u] = ldg4(dY + pt * 4 * ROW + rb * ROW + q4 * 4);
            ra[u] = ldg4(h + pt * ld_h + q4 * 4);
        }
    };
    if (g0 < g1) fetch(g0);
    for (int grp = g0; grp < g1; ++grp) {
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            const int f = tid + 256 * u, pl = f / 96, q4 = f % 96;
            const float vd[4] = {rd[u].x, rd[u].y, rd[u].z, rd[u].w}, va[4] = {ra[u].x, ra[u].y, ra[u].z, ra[u].w};
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int el = 4 * q4 + w, m = el / 3, xyz = el % 3;
                ds[(xyz * 16 + pl) * kSeDwLd + m] = vd[w];
                as[(xyz * 16 + pl) * kSeDwLd + m] = va[w];
            }
        }
        __syncthreads();
        if (grp + 1 < g1) fetch(grp + 1);
#pragma unroll
        for (int kk = 0; kk < 12; ++kk) {
            const float a0 = ds[(4 * kk + lk) * kSeDwLd + 32 * wave + li], a1 = ds[(4 * kk + lk) * kSeDwLd + 32 * wave + 16 + li];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float bv = as[(4 * kk + lk) * kSeDwLd + 16 * j + li];
                acc[0][j] = mfma16(a0, bv, acc[0][j]);
                acc[1][j] = mfma16(a1, bv, acc[1][j]);
            }
        }
        __syncthreads();
    }
    float *Cp = pw + ((size_t)rb * splits + split) * C * C;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) Cp[(size_t)(32 * wave + 16 * i + 4 * lk + r) * C + 16 * j + li] = acc[i][j][r];
}
// partials in split order (float64), then dWf[:, :C] = dW'_0 - dW'_1, dWf[:, C:] = dW'_1 and the same for Wd with dW'_2, dW'_3
__global__ void __launch_bounds__(256) se_dw_finish_kernel(const float *pw, int splits, float *gwf, float *gwd) {
    constexpr int C = 128;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= C * C) return;
    double s[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        double t = 0.0;
        for (int k = 0; k < splits; ++k) t += (double)pw[((size_t)rb * splits + k) * C * C + e];
        s[rb] = t;
    }
    const int m = e / C, k = e % C;
    gwf[(size_t)m * 2 * C + k] = (float)(s[0] - s[1]); gwf[(size_t)m * 2 * C + C + k] = (float)s[1];
    gwd[(size_t)m * 2 * C + k] = (float)(s[2] - s[3]); gwd[(size_t)m * 2 * C + C + k] = (float)s[3];
}

// ---- conv_c backwards ---------------------------------------------------------------------------------------------------------
struct SeHeadBwdArgs {
    const float *hcat, *wf, *wd, *bn_g, *bn_b, *pd;   // as SeHeadArgs
    const double *stats, *S;
    const float *dOut;       // [B][LAT][3]
    float *gpd;              // [P][LAT + 1][3]: g_p rows, then g_d summed over the rows
    float *dhcat;            // [P][KC][3]
    int *mask;               // null, or [P][kSeCh]: 1 where row m of the point took the branch dot < 0 (diagnostic)
    int n_total, N, KC, LAT;
};
SM_DEV SeVnGrad se_head_grad(const SeHeadBwdArgs &a, int pt, int m, bool with_sums) {
    const float *pp = a.pd + ((size_t)pt * (a.LAT + 1) + m) * 3, *dd = a.pd + ((size_t)pt * (a.LAT + 1) + a.LAT) * 3;
    const float *up = a.dOut + ((size_t)(pt / a.N) * a.LAT + m) * 3;
    const float p[3] = {pp[0], pp[1], pp[2]}, d[3] = {dd[0], dd[1], dd[2]}, go[3] = {up[0] / a.N, up[1] / a.N, up[2] / a.N};
    const float mean = (float)a.stats[m], rstd = 1.0f / sqrtf((float)a.stats[kSeCh + m] + 1e-5f);
    const float m1 = with_sums ? (float)(a.S[m] / (double)a.n_total) : 0.f, m2 = with_sums ? (float)(a.S[kSeCh + m] / (double)a.n_total) : 0.f;
    return se_vn_grad(p, d, mean, rstd, a.bn_g[m], a.bn_b[m], go, m1, m2);
}
__global__ void se_head_bwd_sums_kernel(SeHeadBwdArgs a, double *part) {
    const int m = threadIdx.x;
    if (m >= a.LAT) return;
    double s1 = 0.0, s2 = 0.0;
    for (int pt = blockIdx.x; pt < a.n_total; pt += gridDim.x) {
        const SeVnGrad v = se_head_grad(a, pt, m, false);
        s1 += (double)v.gs; s2 += (double)v.gs * (double)v.xh;
    }
    double *dst = part + (size_t)blockIdx.x * kSePartQ * kSeCh;
    dst[m] = s1; dst[kSeCh + m] = s2;
}
// one workgroup per point: g_p of every row, g_d added over the rows in row order; then dhcat = Wf^T g_p + wd (x) g_d
__global__ void __launch_bounds__(256) se_head_bwd_point_kernel(SeHeadBwdArgs a) {
    __shared__ float gps[256 * 3], gds[256 * 3], gdt[3];
    const int pt = blockIdx.x, m = threadIdx.x;
    if (m < a.LAT) {
        const SeVnGrad v = se_head_grad(a, pt, m, true);
        if (a.mask) a.mask[(size_t)pt * kSeCh + m] = (int)v.neg;
#pragma unroll
        for (int k = 0; k < 3; ++k) { gps[m * 3 + k] = v.gp[k]; gds[m * 3 + k] = v.gd[k]; a.gpd[((size_t)pt * (a.LAT + 1) + m) * 3 + k] = v.gp[k]; }
    }
    __syncthreads();
    if (m < 3) {
        float s = 0.f;
        for (int r = 0; r < a.LAT; ++r) s += gds[r * 3 + m];
        gdt[m] = s;
        a.gpd[((size_t)pt * (a.LAT + 1) + a.LAT) * 3 + m] = s;
    }
    __syncthreads();
    for (int c = m; c < a.KC; c += 256) {
        const float w = a.wd[c];
        float o[3] = {w * gdt[0], w * gdt[1], w * gdt[2]};
        for (int r = 0; r < a.LAT; ++r) {
            const float wr = a.wf[(size_t)r * a.KC + c];
            o[0] = fmaf(wr, gps[r * 3], o[0]); o[1] = fmaf(wr, gps[r * 3 + 1], o[1]); o[2] = fmaf(wr, gps[r * 3 + 2], o[2]);
        }
        float *dst = a.dhcat + ((size_t)pt * a.KC + c) * 3;
        dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    }
}
// dWf[m][c] = sum_pt g_p[pt][m].hcat[pt][c] (row LAT: dwd[c]): one thread per element and split, the split's points in order
// ph [splits][(LAT + 1) KC] float64
__global__ void __launch_bounds__(256) se_head_bwd_dw_kernel(SeHeadBwdArgs a, int per_split, double *ph) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, n_el = (int64_t)(a.LAT + 1) * a.KC;
    if (e >= n_el) return;
    const int m = (int)(e / a.KC), c = (int)(e % a.KC);
    const int p0 = blockIdx.y * per_split, p1 = min(p0 + per_split, a.n_total);
    double s = 0.0;
    for (int pt = p0; pt < p1; ++pt) {
        const float *gp = a.gpd + ((size_t)pt * (a.LAT + 1) + m) * 3, *hp = a.hcat + ((size_t)pt * a.KC + c) * 3;
        s += (double)gp[0] * hp[0] + (double)gp[1] * hp[1] + (double)gp[2] * hp[2];
    }
    ph[(size_t)blockIdx.y * n_el + e] = s;
}
__global__ void __launch_bounds__(256) se_head_bwd_dw_finish_kernel(const double *ph, int splits, int LAT, int KC, float *gwf, float *gwd) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, n_el = (int64_t)(LAT + 1) * KC;
    if (e >= n_el) return;
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += ph[(size_t)k * n_el + e];
    if (e < (int64_t)LAT * KC) gwf[e] = (float)s; else gwd[e - (int64_t)LAT * KC] = (float)s;
}

// ---- the weight images from the flat parameter vector (shapemol_se_create, shapemol_se_load_weights) ----------------------------
// The library's one packer: plain copies, and per block W' = [Wf1 ; Wf2 - Wf1 ; Wd1 ; Wd2 - Wd1] as A fragments of se_point_linear_kernel.
struct SeLoadArgs {
    const float *src; float *dst;
    int L, LAT;
    unsigned o_pos_wf, o_pos_g, o_pos_b, o_pos_wd, o_c_wf, o_c_g, o_c_b, o_c_wd;
    unsigned o_img[8], o_g[8], o_b[8];
};
__global__ void __launch_bounds__(256) se_load_weights_kernel(SeLoadArgs a) {
    constexpr unsigned C = 128, BLK = 4 * C * C + 2 * C;
    const unsigned n = 6 * C + a.L * BLK + a.LAT * a.L * C + 2 * a.LAT + a.L * C;
    unsigned i = blockIdx.x * 256 + threadIdx.x;                  // index of a DESTINATION element, the segments in the source's order
    if (i >= n) return;
    if (i < 6 * C) {
        const unsigned o = i < 2 * C ? a.o_pos_wf + i : i < 3 * C ? a.o_pos_g + (i - 2 * C) : i < 4 * C ? a.o_pos_b + (i - 3 * C) : a.o_pos_wd + (i - 4 * C);
        a.dst[o] = a.src[i];
        return;
    }
    i -= 6 * C;
    if (i < a.L * BLK) {
        const unsigned l = i / BLK, e = i % BLK;
        const float *s = a.src + 6 * C + (size_t)l * BLK, *wf = s, *wd = s + 2 * C * C + 2 * C;
        if (e < 4 * C * C) {
            const unsigned r = e & 3, lane = (e >> 2) & 63, ts = e >> 8, s4 = ts % (C / 16), t = ts / (C / 16);
            const unsigned row = 16 * t + (lane & 15), col = 4 * (4 * s4 + r) + (lane >> 4), part = row / C, m = row % C;
            const float *w = part < 2 ? wf : wd;
            a.dst[a.o_img[l] + e] = (part & 1) ? w[(size_t)m * 2 * C + C + col] - w[(size_t)m * 2 * C + col] : w[(size_t)m * 2 * C + col];
        } else {
            const unsigned k = e - 4 * C * C;
            a.dst[k < C ? a.o_g[l] + k : a.o_b[l] + (k - C)] = s[2 * C * C + k];
        }
        return;
    }
    i -= a.L * BLK;
    const float *s = a.src + 6 * C + (size_t)a.L * BLK;
    const unsigned nwf = a.LAT * a.L * C;
    const unsigned o = i < nwf ? a.o_c_wf + i : i < nwf + a.LAT ? a.o_c_g + (i - nwf) : i < nwf + 2 * a.LAT ? a.o_c_b + (i - nwf - a.LAT) : a.o_c_wd + (i - nwf - 2 * a.LAT);
    a.dst[o] = s[i];
}
