// Batches for the shape auto-encoder, built on the device from triangle meshes: the reference's ShapeData / collate_fn
// (datasets/shape_data.py:106-187) and the mesh half of get_pointAE_shape_emb (utils/shape.py:240-284).  Per mesh:
//   surface cloud   P points, area-weighted (pytorch3d's sample_points_from_meshes): three uniforms (u0, u1, u2) per point;
//                   the face is the first k with cdf[k] > u0 * cdf[F - 1] (cdf: the host's sequential running sum of the
//                   float64 face areas), the point (w0 A + w1 B) + w2 C with s = sqrt(u1), w0 = 1 - s, w1 = s (1 - u2),
//                   w2 = s u2, rounded to float32 -- pytorch3d's clouds are float32 and everything below sees the rounded cloud
//   candidates      3T query points ((u * ((hi - lo) + 2)) + lo) - 1 per coordinate, lo / hi the vertex bounding box
//                   (np.random.random((3T, 3)) * (mesh.extents + 2) + mesh.bounds[0] - 1)
//   face image      the projected faces and their boxes that mesh_contains reads, built on the device from the uploaded
//                   vertices and face indices (what mesh_image of sm_guide_host.h builds on the host)
//   classify        per candidate: inside the mesh (mesh_contains of sm_mesh.h: this project's ray parity, not trimesh's) and the
//                   distance to the nearest point of the un-centred float32 cloud (mesh_cloud_d2, float64)
//   select          n_in = min(T / 2, #inside) and n_out = T - n_in: the FIRST n_in inside candidates in candidate order, then
//                   the first n_out outside candidates in candidate order; signed distance +d / -d, or occupancy 1 / 0
//   centre          offset = float32(sum of the float32 cloud in float64 / P); cloud - offset in float32, the query points
//                   float32(p - offset) from their float64 values, the vertex bounding box minus offset
// All arithmetic is float64 without contraction, so tests/shape_data_oracle.py restates it operation for operation.
// Uniforms: fed tables (cloud_draws [B][P][3], query_draws [B][3T][3], float64) or Philox keyed by (seed; point, shape, tag),
// tags 300, 301 for the cloud and 310, 311 for the candidates (the guidance kernels use 100 + j and 200 + j), 53 bits each as
// mesh_pull_kernel makes them.
#pragma once
#include "sm_device.h"
// sm_mesh.h and the sm_misc.h behind it define their kernels in the library's main translation unit as well: this one takes
// them with internal linkage (it launches none of them; what it calls are their device functions)
namespace {
#include "sm_mesh.h"
}

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

constexpr int kSdataMaxCloud = 2048;      // the cloud is staged in LDS beside the face tile, as in mesh guidance
constexpr unsigned kSdataPhiloxKey = 0x5da7u;

struct SdataArgs {
    // the meshes, back to back (vert_off, face_off [B + 1]): uploaded
    const double *verts;                  // [V][3]
    const int *face_ix;                   // [F][3] indices into the mesh's own vertices
    const int *vert_off;                  // [B + 1]
    const double *cdf;                    // [F] running sum of the areas, per mesh
    // the face image, built on the device (sdata_image_kernel)
    MeshFace *faces;                      // [F] projected faces
    double4 *fbox;                        // [F] their boxes
    const double *pbounds;                // [B][5] (umin, umax, vmin, vmax, wmax) of every projected mesh
    const double *lohi;                   // [B][6] vertex bounding box (lo xyz, hi xyz)
    const int *face_off;                  // [B + 1]
    const double *cloud_draws, *query_draws;   // fed uniforms or nullptr
    unsigned long long seed;
    // workspace
    float *cloud32;                       // [B][P][3] the un-centred float32 cloud
    double *cand;                         // [B][3T][3]
    double *dist;                         // [B][3T]
    int *flag;                            // [B][3T] 1: inside
    int *counts;                          // [B][2] (inside, outside) candidates
    // outputs (face_idx, flag_out, sel: optional)
    float *cloud_out, *points, *values, *centres, *bounds;
    int *face_idx, *flag_out, *sel;
    int B, P, T, occupancy;
};

#ifndef SM_SHAPE_DATA_HOST_ONLY       // (a host program that wants the image builder alone defines it: no kernel, no device code to link)
SM_DEV double sdata_u53(const uint32_t (&r)[4], int k) {
    return ((double)(r[2 * k] >> 5) * 67108864.0 + (double)(r[2 * k + 1] >> 6)) * (1.0 / 9007199254740992.0);
}
// the three uniforms of point `i` of shape `b`: row i of the shape's fed table, or Philox calls tag, tag + 1
SM_DEV void sdata_draw3(const double *table, size_t row, unsigned long long seed, int b, int i, int tag, double (&u)[3]) {
    if (table) {
        u[0] = table[row * 3]; u[1] = table[row * 3 + 1]; u[2] = table[row * 3 + 2];
    } else {
        Philox ph{(uint32_t)seed, (uint32_t)(seed >> 32)};
        uint32_t r[4];
        ph((uint32_t)i, (uint32_t)b, (uint32_t)tag, kSdataPhiloxKey, r);
        u[0] = sdata_u53(r, 0); u[1] = sdata_u53(r, 1);
        ph((uint32_t)i, (uint32_t)b, (uint32_t)(tag + 1), kSdataPhiloxKey, r);
        u[2] = sdata_u53(r, 0);
    }
}

// The face image of mesh guidance (mesh_image of sm_guide_host.h), one thread per face; grid (ceil(max F / 256), B): the
// projected vertices of the face by the same mesh_project, the canonical-edge bits, the projected box
__global__ void __launch_bounds__(256) sdata_image_kernel(SdataArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, f0 = a.face_off[b], fl = blockIdx.x * 256 + threadIdx.x;
    if (fl >= a.face_off[b + 1] - f0) return;
    const int f = f0 + fl;
    const int ix[3] = {a.face_ix[f * 3], a.face_ix[f * 3 + 1], a.face_ix[f * 3 + 2]};
    const double *V = a.verts + (size_t)a.vert_off[b] * 3;
    MeshFace m;
    double4 bb = make_double4(INFINITY, -INFINITY, INFINITY, -INFINITY);
    m.canon = 0; m.pad = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double *p = V + (size_t)ix[k] * 3;
        mesh_project(p[0], p[1], p[2], m.u[k], m.v[k], m.w[k]);
        if (ix[k] < ix[k == 2 ? 0 : k + 1]) m.canon |= 1 << k;
        bb.x = fmin(bb.x, m.u[k]); bb.y = fmax(bb.y, m.u[k]); bb.z = fmin(bb.z, m.v[k]); bb.w = fmax(bb.w, m.v[k]);
    }
    a.faces[f] = m;
    a.fbox[f] = bb;
}

// one thread per cloud point; grid (ceil(P / 256), B)
__global__ void __launch_bounds__(256) sdata_cloud_kernel(SdataArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.P) return;
    const int f0 = a.face_off[b], F = a.face_off[b + 1] - f0;
    const size_t row = (size_t)b * a.P + i;
    double u[3];
    sdata_draw3(a.cloud_draws, row, a.seed, b, i, 300, u);
    const double *cdf = a.cdf + f0;
    const double x = u[0] * cdf[F - 1];
    int lo = 0, hi = F - 1;                                    // first k with cdf[k] > x (the last face if there is none)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > x) hi = mid; else lo = mid + 1;
    }
    const int *ix = a.face_ix + (size_t)(f0 + lo) * 3;
    const double *V = a.verts + (size_t)a.vert_off[b] * 3;
    const double *A = V + (size_t)ix[0] * 3, *Bv = V + (size_t)ix[1] * 3, *Cv = V + (size_t)ix[2] * 3;
    const double s = sqrt(u[1]);
    const double w0 = 1.0 - s, w1 = s * (1.0 - u[2]), w2 = s * u[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) a.cloud32[row * 3 + k] = (float)((w0 * A[k] + w1 * Bv[k]) + w2 * Cv[k]);
    if (a.face_idx) a.face_idx[row] = lo;
}

// 16 lanes per candidate, 16 candidates per workgroup; grid (ceil(3T / 16), B).  LDS: mesh_lds_bytes(P)
__global__ void __launch_bounds__(256) sdata_classify_kernel(SdataArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double sdata_lds[];
    const int b = blockIdx.y, Q = 3 * a.T, l16 = threadIdx.x & 15;
    const int q_raw = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool ok = q_raw < Q;
    const int q = ok ? q_raw : Q - 1;
    double *cloud = sdata_lds;
    double4 *tile = reinterpret_cast<double4 *>(sdata_lds + mesh_tile_off(a.P));
    const float *c32 = a.cloud32 + (size_t)b * a.P * 3;
    for (int i = threadIdx.x; i < a.P * 3; i += 256) cloud[i] = (double)c32[i];
    __syncthreads();
    const size_t row = (size_t)b * Q + q;
    double u[3], p[3];
    sdata_draw3(a.query_draws, row, a.seed, b, q, 310, u);
    const double *bx = a.lohi + 6 * b;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = ((u[k] * ((bx[3 + k] - bx[k]) + 2.0)) + bx[k]) - 1.0;
    const double d = sqrt(mesh_cloud_d2(cloud, a.P, p, l16));
    MeshGuideArgs v{};
    const int f0 = a.face_off[b];
    v.faces = a.faces + f0; v.fbox = a.fbox + f0; v.n_faces = a.face_off[b + 1] - f0;
    const double *pb = a.pbounds + 5 * b;
    v.umin = pb[0]; v.umax = pb[1]; v.vmin = pb[2]; v.vmax = pb[3]; v.wmax = pb[4];
    const bool inside = mesh_contains(v, tile, p, ok, l16);
    if (ok && l16 == 0) {
        a.cand[row * 3] = p[0]; a.cand[row * 3 + 1] = p[1]; a.cand[row * 3 + 2] = p[2];
        a.dist[row] = d;
        a.flag[row] = inside ? 1 : 0;
        if (a.flag_out) a.flag_out[row] = inside ? 1 : 0;
    }
}

// One workgroup of 256 per shape: the centring, then the ordered selection.
// Sum of the cloud: thread t adds the points t, t + 256, ... in ascending order, then the 256 partial sums fold in halves
// (v[t] += v[t + s], s = 128 .. 1): a fixed order.  Selection: a block prefix scan over the 3T flags, 256 at a time with a
// carried prefix; the rank of a candidate among the inside (outside) ones is its row in the inside (outside) block.
__global__ void __launch_bounds__(256) sdata_finish_kernel(SdataArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[3][256];
    __shared__ float off_s[3];
    __shared__ int wsum[4], tot_s;
    const int b = blockIdx.x, t = threadIdx.x, P = a.P, T = a.T, Q = 3 * T;
    const float *c32 = a.cloud32 + (size_t)b * P * 3;
    double s3[3] = {0.0, 0.0, 0.0};
    for (int i = t; i < P; i += 256) { s3[0] += (double)c32[i * 3]; s3[1] += (double)c32[i * 3 + 1]; s3[2] += (double)c32[i * 3 + 2]; }
    red[0][t] = s3[0]; red[1][t] = s3[1]; red[2][t] = s3[2];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { red[0][t] += red[0][t + s]; red[1][t] += red[1][t + s]; red[2][t] += red[2][t + s]; }
        __syncthreads();
    }
    if (t < 3) {
        const float o = (float)(red[t][0] / (double)P);
        off_s[t] = o;
        a.centres[b * 3 + t] = o;
        a.bounds[(b * 3 + t) * 2] = (float)(a.lohi[6 * b + t] - (double)o);
        a.bounds[(b * 3 + t) * 2 + 1] = (float)(a.lohi[6 * b + 3 + t] - (double)o);
    }
    __syncthreads();
    const float off[3] = {off_s[0], off_s[1], off_s[2]};
    float *co = a.cloud_out + (size_t)b * P * 3;
    for (int i = t; i < P * 3; i += 256) co[i] = c32[i] - off_s[i % 3];
    if (T == 0) return;                                         // clouds only (get_pointAE_shape_emb)
    const int *flag = a.flag + (size_t)b * Q;
    int n = 0;
    for (int i = t; i < Q; i += 256) n += flag[i];
    for (int m = 1; m < 64; m <<= 1) n += __shfl_xor(n, m, 64);
    if ((t & 63) == 0) wsum[t >> 6] = n;
    __syncthreads();
    if (t == 0) tot_s = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    __syncthreads();
    const int tot_in = tot_s, n_in = min(T / 2, tot_in), n_out = T - n_in;
    if (t == 0) { a.counts[2 * b] = tot_in; a.counts[2 * b + 1] = Q - tot_in; }
    const double *cand = a.cand + (size_t)b * Q * 3, *dist = a.dist + (size_t)b * Q;
    float *pts = a.points + (size_t)b * T * 3, *val = a.values + (size_t)b * T;
    int carry = 0;                                              // inside candidates before this pass
    for (int base = 0; base < Q; base += 256) {
        const int i = base + t;
        const bool live = i < Q, in = live && flag[i] != 0;
        const unsigned long long bal = __ballot(in);
        const int lane = t & 63, wave = t >> 6;
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();                                        // wsum of the pass before has been read
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int wpre = 0;
        for (int w = 0; w < wave; ++w) wpre += wsum[w];
        const int rank_in = carry + wpre + before, rank_out = i - rank_in;
        carry += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        const int r = !live ? -1 : in ? (rank_in < n_in ? rank_in : -1) : (rank_out < n_out ? n_in + rank_out : -1);
        if (r >= 0) {
            const double d = dist[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) pts[r * 3 + k] = (float)(cand[i * 3 + k] - (double)off[k]);
            val[r] = a.occupancy ? (in ? 1.0f : 0.0f) : (float)(in ? d : -d);
            if (a.sel) a.sel[(size_t)b * T + r] = i;
        }
    }
}

#endif  // SM_SHAPE_DATA_HOST_ONLY

// ---- host side: validation and what the host uploads for a batch of meshes ----------------------------------------------
// [verts V x 3 | face indices F x 3 | cdf F | projected bounds B x 5 | bounding boxes B x 6 | face_off B + 1 | vert_off B + 1],
// every piece on a 256-byte boundary: 32 bytes per face and 24 per vertex.  The area of a face is 0.5 |(B - A) x (C - A)|, the
// cdf their sequential running sum per mesh; the projected bounds (the early-out of mesh_contains) are those of mesh_image
// (sm_guide_host.h): over the vertices the faces name, projected with mesh_project.  The projected faces and their boxes are
// built on the device (sdata_image_kernel).
struct SdataImage {
    std::vector<unsigned char> bytes;
    size_t o_verts = 0, o_ix = 0, o_cdf = 0, o_pb = 0, o_lohi = 0, o_off = 0, o_voff = 0;
    int64_t F = 0, max_faces = 0;
    int B = 0;
};

// the argument checks (no device is touched); an empty string when all is well
inline std::string sdata_check(int64_t n_shapes, const int64_t *vert_off, const double *verts, const int64_t *face_off, const int32_t *faces,
                               int64_t P, int64_t T, int loss_type) {
    const std::string me = "shape data: ";
    if (n_shapes < 1 || n_shapes > 65535) return me + "n_shapes must be in 1..65535, got " + std::to_string(n_shapes);
    if (!vert_off || !verts || !face_off || !faces) return me + "offsets, vertices and faces are required";
    if (P < 1) return me + "point_cloud_samples must be >= 1, got " + std::to_string(P);
    if (P > kSdataMaxCloud) return me + "point_cloud_samples must be <= 2048 (the cloud is staged in LDS), got " + std::to_string(P);
    if (T != 0 && T < 2) return me + "num_samples must be >= 2, got " + std::to_string(T);
    if (T > (1 << 24)) return me + "num_samples must be <= 2^24, got " + std::to_string(T);
    if (loss_type != 0 && loss_type != 1) return me + "loss_type must be 0 (signed_distance) or 1 (occupancy), got " + std::to_string(loss_type);
    if (vert_off[0] != 0 || face_off[0] != 0) return me + "the vertex and face offsets must start at 0";
    for (int64_t b = 0; b < n_shapes; ++b) {
        const std::string sh = me + "shape " + std::to_string(b) + ": ";
        const int64_t nv = vert_off[b + 1] - vert_off[b], nf = face_off[b + 1] - face_off[b];
        if (nv < 0 || nf < 0) return sh + "the offsets decrease";
        if (nf < 1) return sh + "the mesh needs at least 1 face";
        if (nv > (1 << 26)) return sh + "the mesh has more than 2^26 vertices";
        for (int64_t i = vert_off[b] * 3; i < vert_off[b + 1] * 3; ++i)
            if (!std::isfinite(verts[i])) return sh + "a vertex is not finite";
        for (int64_t i = face_off[b] * 3; i < face_off[b + 1] * 3; ++i)
            if (faces[i] < 0 || faces[i] >= nv) return sh + "face " + std::to_string(i / 3 - face_off[b]) + " names a vertex outside [0, n_verts)";
    }
    if (face_off[n_shapes] > (1 << 27) || vert_off[n_shapes] > (1 << 27)) return me + "more than 2^27 faces or vertices in the batch";
    if (n_shapes * P > (1 << 27) || n_shapes * 3 * T > (1 << 27)) return me + "more than 2^27 cloud points or candidates in the batch";
    return "";
}

// arguments as sdata_check accepts them
inline void sdata_image(int n_shapes, const int64_t *vert_off, const double *verts, const int64_t *face_off, const int32_t *faces, SdataImage &im) {
#pragma clang fp contract(off)
    const size_t F = (size_t)face_off[n_shapes], V = (size_t)vert_off[n_shapes], B = (size_t)n_shapes;
    size_t end = 0;
    auto put = [&](size_t n) { const size_t o = (end + 255) & ~size_t(255); end = o + n; return o; };
    im.o_verts = put(V * 24); im.o_ix = put(F * 12); im.o_cdf = put(F * 8);
    im.o_pb = put(B * 40); im.o_lohi = put(B * 48); im.o_off = put((B + 1) * sizeof(int)); im.o_voff = put((B + 1) * sizeof(int));
    im.bytes.resize(end);                          // (the gaps between the pieces are never read)
    im.F = (int64_t)F; im.B = n_shapes; im.max_faces = 0;
    unsigned char *base = im.bytes.data();
    std::memcpy(base + im.o_verts, verts, V * 24);
    std::memcpy(base + im.o_ix, faces, F * 12);
    double *cdf = reinterpret_cast<double *>(base + im.o_cdf);
    double *pb = reinterpret_cast<double *>(base + im.o_pb), *lohi = reinterpret_cast<double *>(base + im.o_lohi);
    int *off = reinterpret_cast<int *>(base + im.o_off), *voff = reinterpret_cast<int *>(base + im.o_voff);
    std::vector<double> pu, pv, pw;
    for (int b = 0; b < n_shapes; ++b) {
        const int64_t v0 = vert_off[b], nv = vert_off[b + 1] - v0;
        const double *P = verts + v0 * 3;
        off[b] = (int)face_off[b]; voff[b] = (int)v0;
        im.max_faces = std::max(im.max_faces, face_off[b + 1] - face_off[b]);
        pu.resize(nv); pv.resize(nv); pw.resize(nv);
        double *bx = lohi + 6 * b;
        for (int k = 0; k < 3; ++k) { bx[k] = INFINITY; bx[3 + k] = -INFINITY; }
        for (int64_t i = 0; i < nv; ++i) {
            mesh_project(P[i * 3], P[i * 3 + 1], P[i * 3 + 2], pu[i], pv[i], pw[i]);
            for (int k = 0; k < 3; ++k) { bx[k] = std::min(bx[k], P[i * 3 + k]); bx[3 + k] = std::max(bx[3 + k], P[i * 3 + k]); }
        }
        double *bd = pb + 5 * b;
        bd[0] = bd[2] = INFINITY; bd[1] = bd[3] = bd[4] = -INFINITY;
        double run = 0.0;
        for (int64_t f = face_off[b]; f < face_off[b + 1]; ++f) {
            const int32_t *ix = faces + f * 3;
            for (int k = 0; k < 3; ++k) {
                bd[0] = std::min(bd[0], pu[ix[k]]); bd[1] = std::max(bd[1], pu[ix[k]]);
                bd[2] = std::min(bd[2], pv[ix[k]]); bd[3] = std::max(bd[3], pv[ix[k]]);
                bd[4] = std::max(bd[4], pw[ix[k]]);
            }
            const double *A = P + (int64_t)ix[0] * 3, *Bv = P + (int64_t)ix[1] * 3, *Cv = P + (int64_t)ix[2] * 3;
            const double e1[3] = {Bv[0] - A[0], Bv[1] - A[1], Bv[2] - A[2]}, e2[3] = {Cv[0] - A[0], Cv[1] - A[1], Cv[2] - A[2]};
            const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
            run = run + 0.5 * std::sqrt((cx * cx + cy * cy) + cz * cz);
            cdf[f] = run;
        }
    }
    off[n_shapes] = (int)face_off[n_shapes]; voff[n_shapes] = (int)vert_off[n_shapes];
}
