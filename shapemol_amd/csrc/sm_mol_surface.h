// Molecular surface meshes on the device from atom centres and radii: what the reference's get_mesh (utils/shape.py:153-162)
// asks of oddt, under THIS project's rule (oddt is not available to compare with).  Per molecule, float64:
//   grid        lo = min c - (r_max + p) - 2h per axis, n = ceil((max c + r_max + p + 2h - lo) / h) + 1 nodes; node (a, b, c) at
//               lo + h (a, b, c), linear index (a ny + b) nz + c.  The outer two layers lie outside: the surface is closed
//   field       fA(x) = min_i (|x - c_i| - (r_i + p)); O = {fA >= 0}
//   erosion     p == 0: g = fA.  Else g = p - min(d(x, O), p + h), d the distance to the nearest NODE of O within
//               R = ceil((p + h) / h) nodes each way (a node of O further out is further than p + h).  d = h sqrt(m) with m the
//               smallest di^2 + dj^2 + dk^2: the search works on integers over a one-byte-per-node LDS tile with a halo of R, and
//               takes d from the host's table of min(h sqrt(m), p + h) -- no 8-byte LDS traffic, no device sqrt behind a sign
//   surface     zero level of g (g >= 0: outside) by marching tetrahedra on the six Kuhn tetrahedra 0 -> e_i -> e_i + e_j -> 7 of
//               every cell: no ambiguous case, watertight for any field.  A vertex lies on one of seven edge classes of its
//               lower node (x, y, z; xy, xz, yz; xyz) at t = g0 / (g0 - g1); normals point from g < 0 to g >= 0
//   order       vertex ids: exclusive scan of the cut-edge flags in (node, class) order; face ids: scan of the per-cell triangle
//               counts in (cell, tetrahedron, triangle) order.  No atomic decides anything: two runs give the same arrays
// Kernels: field, erode, count (edge masks, triangle counts, sums per scan block), scan (block sums per molecule), verts, faces.
// Limits (refused on the host before any launch): kMsurfMaxNodes nodes per molecule, kMsurfMaxBatchNodes per call,
// kMsurfMaxAtoms atoms per molecule (staged in LDS), stencil R <= kMsurfMaxStencil (the tile with its halo fits 64 KiB of LDS);
// with them a molecule has < 2^31 / 7 nodes, so int32 holds every vertex and face index.
// tests/mol_surface_oracle.py restates all of it in numpy.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#pragma clang fp contract(off)

constexpr int kMsurfMaxNodes = 128 * 128 * 128;          // 19 bytes of workspace each; 1 A spacing: 120 A, 0.25 A: 30 A across
constexpr int64_t kMsurfMaxBatchNodes = 1ll << 26;       // 1.2 GiB of workspace
constexpr int kMsurfMaxAtoms = 1024;                     // 32 KiB of LDS in the field kernel
constexpr int kMsurfMaxStencil = 16;                     // (8 + 2 * 16)^3 = 64000 bytes of LDS in the erosion kernel
constexpr int kMsurfTile = 8;                            // erosion tile: 8 x 8 x 8 nodes, one thread each
constexpr int kMsurfScanBlock = 1024;                    // nodes per scan block: 256 threads x 4 consecutive nodes
constexpr int kMsurfScanWidth = 256;                     // scan blocks the per-molecule scan takes per pass (its workgroup)
constexpr int kMsurfMaxMols = 65535;                     // gridDim.y

struct MsurfMol {
    double lo[3];
    long long node_off;                   // of its first node in the per-node arrays
    long long vert_off, face_off;         // of its first vertex / face in the outputs (known after the scans)
    int n[3];
    int atom_off, n_atoms;
    int chunk_off, n_chunks;              // scan blocks
    int tiles[3];
};

struct MsurfArgs {
    const MsurfMol *mol;                  // [B]
    const double4 *atoms;                 // (x, y, z, r + p)
    const double *dtab;                   // [3 R^2 + 2] min(h sqrt(m), p + h); the last entry (no node of O in reach) = p + h
    double *g;                            // per node
    unsigned char *outside;               // per node: fA >= 0 (p > 0 only)
    unsigned char *emask;                 // per node: its cut edges, bit = class
    unsigned char *ntri;                  // per node as a cell's lower corner: triangles of the cell
    int *vbase;                           // per node: id of its first vertex
    unsigned long long *chunk;            // per scan block: (vertices | triangles << 32), after the scan kernel exclusive
    int *counts;                          // [B][2] vertices, faces
    double *verts;                        // [sum V][3]
    int *faces;                           // [sum F][3]
    double h, p;
    int R;
};

__device__ __constant__ unsigned char kMsurfKuhn[6][4] = {{0, 1, 3, 7}, {0, 5, 1, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 6, 4, 7}};
// per case (bit i: corner i of a positively oriented tetrahedron has g < 0): triangle count << 24 | triangles of three edges,
// an edge = 4 bits (i << 2 | j)
__device__ __constant__ unsigned kMsurfTri[16] = {0x0000000u, 0x1000321u, 0x1000674u, 0x2672732u, 0x1000b98u, 0x2b93913u, 0x28b4b74u, 0x1000edcu,
                                                  0x1000decu, 0x2de1e21u, 0x2ec6c46u, 0x10009b8u, 0x2cd8d98u, 0x1000764u, 0x1000231u, 0x0000000u};
__device__ __constant__ unsigned char kMsurfEdgeUpper[7] = {1, 2, 4, 3, 5, 6, 7};      // class -> upper corner
__device__ __constant__ unsigned char kMsurfEdgeClass[8] = {0, 0, 1, 3, 2, 4, 5, 6};   // corner difference -> class

// exclusive scan over the 256 threads of a block (wave64 shuffles, four wave sums through LDS); `total` = the block's sum
__device__ __forceinline__ unsigned long long msurf_block_scan(unsigned long long v, unsigned long long *s_wave, unsigned long long &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                      // s_wave may still be read from a call before
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    unsigned long long base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < w) base += s_wave[i];
        total += s_wave[i];
    }
    return base + inc - v;
}

// signs of the eight corners of the cell whose lower node is (ia, ib, ic): bit k = corner k has g < 0; corners off the grid: 0
__device__ __forceinline__ unsigned msurf_corner_signs(const double *g, const MsurfMol &m, int ia, int ib, int ic, int node) {
    const int ny = m.n[1], nz = m.n[2];
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
        if (ia + dx < m.n[0] && ib + dy < ny && ic + dz < nz) s |= (unsigned)(g[node + (dx * ny + dy) * nz + dz] < 0.0) << k;
    }
    return s;
}

__global__ __launch_bounds__(256) void msurf_field_kernel(MsurfArgs a) {
    __shared__ double4 s_atom[kMsurfMaxAtoms];
    const MsurfMol &m = a.mol[blockIdx.y];
    const int ny = m.n[1], nz = m.n[2], nodes = m.n[0] * ny * nz;
    if ((long long)blockIdx.x * 256 >= nodes) return;
    for (int i = threadIdx.x; i < m.n_atoms; i += 256) s_atom[i] = a.atoms[m.atom_off + i];
    __syncthreads();
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= nodes) return;
    const int ic = node % nz, ib = (node / nz) % ny, ia = node / (nz * ny);
    const double x = m.lo[0] + a.h * (double)ia, y = m.lo[1] + a.h * (double)ib, z = m.lo[2] + a.h * (double)ic;
    double f = INFINITY;
    for (int i = 0; i < m.n_atoms; ++i) {
        const double4 c = s_atom[i];      // one address for the whole wave: a broadcast
        const double dx = x - c.x, dy = y - c.y, dz = z - c.z;
        f = fmin(f, sqrt((dx * dx + dy * dy) + dz * dz) - c.w);
    }
    if (a.p == 0.0) a.g[m.node_off + node] = f;
    else a.outside[m.node_off + node] = f >= 0.0;
}

// One 8^3 tile per workgroup; the flags of the tile and R nodes around it in LDS, one byte each (off the grid: 0).  The 32 lanes
// of a half wave read 4 rows of 8 consecutive bytes: 2 dwords per row, rows W bytes apart, so at most 2 lanes ask one bank for
// different dwords where two rows fall W = 32 or 40 bytes apart -- bytes of one dword are one address.
__global__ __launch_bounds__(512) void msurf_erode_kernel(MsurfArgs a) {
    extern __shared__ unsigned char s_out[];
    const MsurfMol &m = a.mol[blockIdx.y];
    const int n_tiles = m.tiles[0] * m.tiles[1] * m.tiles[2];
    if ((int)blockIdx.x >= n_tiles) return;
    const int R = a.R, W = kMsurfTile + 2 * R;
    const int nx = m.n[0], ny = m.n[1], nz = m.n[2];
    const int tc = blockIdx.x % m.tiles[2], tb = (blockIdx.x / m.tiles[2]) % m.tiles[1], ta = blockIdx.x / (m.tiles[2] * m.tiles[1]);
    const int a0 = ta * kMsurfTile - R, b0 = tb * kMsurfTile - R, c0 = tc * kMsurfTile - R;
    const unsigned char *outside = a.outside + m.node_off;
    for (int i = threadIdx.x; i < W * W * W; i += 512) {
        const int ia = a0 + i / (W * W), ib = b0 + (i / W) % W, ic = c0 + i % W;
        const bool in = ia >= 0 && ia < nx && ib >= 0 && ib < ny && ic >= 0 && ic < nz;
        s_out[i] = in ? outside[(ia * ny + ib) * nz + ic] : (unsigned char)0;
    }
    __syncthreads();
    const int lc = threadIdx.x & 7, lb = (threadIdx.x >> 3) & 7, la = threadIdx.x >> 6;
    const int ia = a0 + R + la, ib = b0 + R + lb, ic = c0 + R + lc;
    if (ia >= nx || ib >= ny || ic >= nz) return;
    int best = 3 * R * R + 1;
    for (int di = -R; di <= R; ++di) {
        const int s1 = di * di;
        if (s1 >= best) continue;
        for (int dj = -R; dj <= R; ++dj) {
            const int s2 = s1 + dj * dj;
            if (s2 >= best) continue;
            const unsigned char *row = s_out + ((la + R + di) * W + (lb + R + dj)) * W + lc + R;
            for (int dk = -R; dk <= R; ++dk) {
                const int s3 = s2 + dk * dk;
                if (s3 < best && row[dk]) best = s3;
            }
        }
    }
    a.g[m.node_off + (ia * ny + ib) * nz + ic] = a.p - a.dtab[best];
}

// per node: its cut edges and, as a cell's lower corner, the cell's triangle count; per scan block the two sums
__global__ __launch_bounds__(256) void msurf_count_kernel(MsurfArgs a) {
    __shared__ unsigned long long s_wave[4];
    const MsurfMol &m = a.mol[blockIdx.y];
    if ((int)blockIdx.x >= m.n_chunks) return;
    const int ny = m.n[1], nz = m.n[2], nodes = m.n[0] * ny * nz;
    const double *g = a.g + m.node_off;
    unsigned long long sum = 0;
    for (int q = 0; q < 4; ++q) {
        const int node = blockIdx.x * kMsurfScanBlock + threadIdx.x * 4 + q;
        if (node >= nodes) break;
        const int ic = node % nz, ib = (node / nz) % ny, ia = node / (nz * ny);
        const unsigned s = msurf_corner_signs(g, m, ia, ib, ic, node);
        unsigned mask = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int up = kMsurfEdgeUpper[k];
            const bool exists = ia + (up & 1) < m.n[0] && ib + ((up >> 1) & 1) < ny && ic + (up >> 2) < nz;
            if (exists && ((s ^ (s >> up)) & 1u)) mask |= 1u << k;
        }
        unsigned tri = 0;
        if (ia + 1 < m.n[0] && ib + 1 < ny && ic + 1 < nz) {
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                unsigned cs = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) cs |= ((s >> kMsurfKuhn[t][i]) & 1u) << i;
                tri += kMsurfTri[cs] >> 24;
            }
        }
        a.emask[m.node_off + node] = (unsigned char)mask;
        a.ntri[m.node_off + node] = (unsigned char)tri;
        sum += (unsigned long long)__popc(mask) | ((unsigned long long)tri << 32);
    }
    unsigned long long total;
    (void)msurf_block_scan(sum, s_wave, total);
    if (threadIdx.x == 0) a.chunk[m.chunk_off + blockIdx.x] = total;
}

// one workgroup per molecule: exclusive scan of its scan blocks' sums in place, 256 at a time with a carry; the totals
__global__ __launch_bounds__(kMsurfScanWidth) void msurf_scan_kernel(MsurfArgs a) {
    __shared__ unsigned long long s_wave[4];
    const MsurfMol &m = a.mol[blockIdx.x];
    unsigned long long carry = 0;
    for (int base = 0; base < m.n_chunks; base += kMsurfScanWidth) {
        const int i = base + threadIdx.x;
        const unsigned long long v = i < m.n_chunks ? a.chunk[m.chunk_off + i] : 0ull;
        unsigned long long total;
        const unsigned long long ex = msurf_block_scan(v, s_wave, total);
        if (i < m.n_chunks) a.chunk[m.chunk_off + i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        a.counts[2 * blockIdx.x] = (int)(carry & 0xffffffffull);
        a.counts[2 * blockIdx.x + 1] = (int)(carry >> 32);
    }
}

__global__ __launch_bounds__(256) void msurf_verts_kernel(MsurfArgs a) {
    __shared__ unsigned long long s_wave[4];
    const MsurfMol &m = a.mol[blockIdx.y];
    if ((int)blockIdx.x >= m.n_chunks) return;
    const int ny = m.n[1], nz = m.n[2], nodes = m.n[0] * ny * nz;
    const int first = blockIdx.x * kMsurfScanBlock + threadIdx.x * 4;
    unsigned mask[4];
    unsigned long long sum = 0;
    for (int q = 0; q < 4; ++q) {
        mask[q] = first + q < nodes ? a.emask[m.node_off + first + q] : 0u;
        sum += __popc(mask[q]);
    }
    unsigned long long total;
    int id = (int)((a.chunk[m.chunk_off + blockIdx.x] & 0xffffffffull) + msurf_block_scan(sum, s_wave, total));
    const double *g = a.g + m.node_off;
    for (int q = 0; q < 4; ++q) {
        const int node = first + q;
        if (node >= nodes) break;
        a.vbase[m.node_off + node] = id;
        if (!mask[q]) continue;
        const int ic = node % nz, ib = (node / nz) % ny, ia = node / (nz * ny);
        const double x0[3] = {m.lo[0] + a.h * (double)ia, m.lo[1] + a.h * (double)ib, m.lo[2] + a.h * (double)ic};
        const double g0 = g[node];
        for (int k = 0; k < 7; ++k) {
            if (!(mask[q] >> k & 1u)) continue;
            const int up = kMsurfEdgeUpper[k], dx = up & 1, dy = (up >> 1) & 1, dz = up >> 2;
            const double g1 = g[node + (dx * ny + dy) * nz + dz];
            const double th = (g0 / (g0 - g1)) * a.h;
            double *v = a.verts + (m.vert_off + id) * 3;
            v[0] = dx ? x0[0] + th : x0[0];
            v[1] = dy ? x0[1] + th : x0[1];
            v[2] = dz ? x0[2] + th : x0[2];
            ++id;
        }
    }
}

__global__ __launch_bounds__(256) void msurf_faces_kernel(MsurfArgs a) {
    __shared__ unsigned long long s_wave[4];
    const MsurfMol &m = a.mol[blockIdx.y];
    if ((int)blockIdx.x >= m.n_chunks) return;
    const int ny = m.n[1], nz = m.n[2], nodes = m.n[0] * ny * nz;
    const int first = blockIdx.x * kMsurfScanBlock + threadIdx.x * 4;
    unsigned tri[4];
    unsigned long long sum = 0;
    for (int q = 0; q < 4; ++q) {
        tri[q] = first + q < nodes ? a.ntri[m.node_off + first + q] : 0u;
        sum += tri[q];
    }
    unsigned long long total;
    long long id = (long long)((a.chunk[m.chunk_off + blockIdx.x] >> 32) + msurf_block_scan(sum, s_wave, total));
    const double *g = a.g + m.node_off;
    const unsigned char *emask = a.emask + m.node_off;
    const int *vbase = a.vbase + m.node_off;
    for (int q = 0; q < 4; ++q) {
        const int node = first + q;
        if (node >= nodes) break;
        if (!tri[q]) continue;            // (a cell off the grid's upper faces has none)
        const int ic = node % nz, ib = (node / nz) % ny, ia = node / (nz * ny);
        const unsigned s = msurf_corner_signs(g, m, ia, ib, ic, node);
        for (int t = 0; t < 6; ++t) {
            unsigned cs = 0;
            for (int i = 0; i < 4; ++i) cs |= ((s >> kMsurfKuhn[t][i]) & 1u) << i;
            const unsigned w = kMsurfTri[cs];
            for (unsigned k = 0; k < (w >> 24); ++k) {
                int *f = a.faces + (m.face_off + id) * 3;
                for (int e = 0; e < 3; ++e) {
                    const unsigned ij = (w >> (12 * k + 4 * e)) & 15u;
                    const unsigned c0 = kMsurfKuhn[t][ij >> 2], c1 = kMsurfKuhn[t][ij & 3u];
                    const unsigned lo = c0 < c1 ? c0 : c1, cls = kMsurfEdgeClass[c0 ^ c1];      // Kuhn edges: one corner holds the other's bits
                    const int ln = node + (int)(((lo & 1u) * ny + ((lo >> 1) & 1u)) * nz + (lo >> 2));
                    f[e] = vbase[ln] + __popc(emask[ln] & ((1u << cls) - 1u));
                }
                ++id;
            }
        }
    }
}

// ---- host: checks and the plan of a batch ----------------------------------------------------------------------------------
struct MsurfPlan {
    std::vector<MsurfMol> mol;
    std::vector<double> atoms;            // [N][4] scaled (x, y, z, r + p)
    std::vector<double> dtab;
    double p = 0, h = 0;                  // scaled probe radius, spacing
    int R = 0;
    long long nodes = 0;
    int chunks = 0, max_nodes = 0, max_chunks = 0, max_tiles = 0;
};

// The arguments and limits of a batch and, with `plan`, its grids.  Empty string: fine.  Host only: no device is touched.
inline std::string msurf_plan(int64_t B, const int64_t *atom_off, const double *centres, const double *radii, double p, double h, double scaling,
                              MsurfPlan *plan) {
    const std::string pre = "molecular surface: ";
    if (B < 1 || B > kMsurfMaxMols) return pre + "the number of molecules must be 1.." + std::to_string(kMsurfMaxMols);
    if (!atom_off || !centres || !radii) return pre + "an input pointer is missing";
    if (!(scaling > 0) || !std::isfinite(scaling)) return pre + "scaling must be positive and finite";
    if (!(p >= 0) || !std::isfinite(p)) return pre + "probe_radius must be >= 0 and finite";
    if (!(h > 0) || !std::isfinite(h)) return pre + "the grid spacing must be positive and finite";
    if (atom_off[0] != 0) return pre + "the atom offsets must start at 0";
    const double ps = p * scaling;
    const double stencil = std::ceil((ps + h) / h);
    if (ps > 0 && stencil > kMsurfMaxStencil)
        return pre + "probe_radius over spacing gives an erosion stencil of " + std::to_string((long long)std::min(stencil, 1e15)) + " nodes; the limit is " +
               std::to_string(kMsurfMaxStencil);
    MsurfPlan pl;
    pl.p = ps; pl.h = h; pl.R = ps > 0 ? (int)stencil : 0;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t lo_i = atom_off[b], n_at = atom_off[b + 1] - atom_off[b];
        const std::string who = pre + "molecule " + std::to_string(b) + ": ";
        if (n_at < 1) return who + "no atoms";
        if (n_at > kMsurfMaxAtoms) return who + std::to_string(n_at) + " atoms; the limit is " + std::to_string(kMsurfMaxAtoms);
        double rmax = 0, cmin[3], cmax[3];
        for (int64_t i = lo_i; i < lo_i + n_at; ++i) {
            const double r = radii[i] * scaling;
            if (!(r > 0) || !std::isfinite(r)) return who + "every radius must be positive and finite";
            rmax = std::max(rmax, r);
            for (int k = 0; k < 3; ++k) {
                const double c = centres[3 * i + k] * scaling;
                if (!std::isfinite(c)) return who + "a coordinate is not finite";
                cmin[k] = i == lo_i ? c : std::min(cmin[k], c);
                cmax[k] = i == lo_i ? c : std::max(cmax[k], c);
            }
            pl.atoms.insert(pl.atoms.end(), {centres[3 * i] * scaling, centres[3 * i + 1] * scaling, centres[3 * i + 2] * scaling, r + ps});
        }
        MsurfMol m{};
        double nodes = 1;
        for (int k = 0; k < 3; ++k) {
            m.lo[k] = (cmin[k] - (rmax + ps)) - 2.0 * h;
            const double n = std::ceil(((((cmax[k] + rmax) + ps) + 2.0 * h) - m.lo[k]) / h) + 1;
            nodes *= n;
            if (!(nodes <= (double)kMsurfMaxNodes))
                return who + "the grid exceeds " + std::to_string(kMsurfMaxNodes) + " nodes (128^3); use a larger spacing";
            m.n[k] = (int)n;
            m.tiles[k] = (m.n[k] + kMsurfTile - 1) / kMsurfTile;
        }
        const int n_nodes = m.n[0] * m.n[1] * m.n[2];
        m.atom_off = (int)lo_i; m.n_atoms = (int)n_at;
        m.node_off = pl.nodes;
        m.chunk_off = pl.chunks;
        m.n_chunks = (n_nodes + kMsurfScanBlock - 1) / kMsurfScanBlock;
        pl.nodes += n_nodes;
        pl.chunks += m.n_chunks;
        pl.max_nodes = std::max(pl.max_nodes, n_nodes);
        pl.max_chunks = std::max(pl.max_chunks, m.n_chunks);
        pl.max_tiles = std::max(pl.max_tiles, m.tiles[0] * m.tiles[1] * m.tiles[2]);
        if (pl.nodes > kMsurfMaxBatchNodes) return pre + "the batch exceeds " + std::to_string(kMsurfMaxBatchNodes) + " grid nodes; split it";
        pl.mol.push_back(m);
    }
    const int big = 3 * pl.R * pl.R + 1;
    pl.dtab.resize((size_t)big + 1);
    for (int mm = 0; mm < big; ++mm) pl.dtab[mm] = std::min(h * std::sqrt((double)mm), ps + h);
    pl.dtab[big] = ps + h;
    if (plan) *plan = std::move(pl);
    return "";
}
