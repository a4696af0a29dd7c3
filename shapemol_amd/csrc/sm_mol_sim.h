// Gaussian similarity of molecules and the rigid overlay that maximises it.
//
// Fixed pose: for a job (molecule x, molecule y) the sum over atom pairs of w_i w_j sum_k A_k exp(-(B_k r2)),
// r2 = (dx*dx + dy*dy) + dz*dz.  shape mode (one term): s = alpha_i + alpha_j, A = (PI15 * (p_i * p_j)) / (s * sqrt(s)),
// B = (alpha_i * alpha_j) / s, w = 1 (shape_tanimoto / VAB_2nd_order of the reference's shaep_utils).  esp mode: K <= 16 terms
// with the caller's A_k, B_k and w = the charges (GaussInt of the reference's espsim; its b are -B_k).  Self overlaps and cross
// overlaps are jobs of the same kernel; a second kernel turns the three integrals of a pair into its score.
//
// Overlay: per (pair, start) a team maximises the shape S_ab over rigid motions of molecule a by BFGS over the 6 rigid degrees
// of freedom, from the four proper rotations that map a's principal frame onto b's (centroids coincident) and, on request,
// from the pose as given.  Value, force on every atom and torque about a's centroid come from one pass over the atom pairs.
//
// Arithmetic: float64, no FMA contraction (the pragma below).  Thread i of a team owns atom i of x and sums over the atoms j of
// y in ascending order; the threads' sums are added by a binary tree over LDS in a fixed order.  No atomics: every output is
// the same bits in every run.
//
// Two launch forms: a team of 64 threads (one wave) when both molecules have at most 64 atoms, a team of 256 threads (the
// workgroup) up to 256 atoms.  A team is a workgroup in both forms.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#pragma clang fp contract(off)

constexpr int kMsimWaveAtoms = 64;                       // wave form: both molecules of a job
constexpr int kMsimMaxAtoms = 256;                       // block form
constexpr int kMsimMaxTerms = 16;                        // esp mode: Gaussians per atom pair
constexpr int kMsimStarts = 4;                           // principal-frame starts; the pose as given is start 4
constexpr int kMsimMaxStarts = kMsimStarts + 1;
constexpr int kMsimMaxIter = 10000;                      // upper limit of the caller's iteration cap
constexpr int kMsimHalvings = 30;                        // step halvings of one line search
constexpr int kMsimSweeps = 12;                          // Jacobi sweeps of the 3x3 eigen-solver
constexpr int kMsimStartDoubles = 16;                    // a start's result: S_ab, R (9), t (3), iterations, converged, moved
constexpr int64_t kMsimMaxMols = 1 << 20, kMsimMaxPairs = 1 << 22;
constexpr double kMsimPi15 = 0x1.645f7c63f2c6bp+2;       // pi ** 1.5 as the reference's Python forms it
constexpr double kMsimStepMax = 0.5;                     // largest component of one step: Angstrom, radian
constexpr double kMsimArmijo = 1e-4;

enum { MSIM_SHAPE = 0, MSIM_ESP = 1 };
enum { MSIM_TANIMOTO = 0, MSIM_CARBO = 1 };

// One integral: the atoms [xo, xo + xn) of position set xs (0: a, 1: b, 2: the overlaid copies of a) with parameters from
// [xp, xp + xn) of parameter set xs & 1, against the same of y; the sum goes to out.
struct MsimJob { int xs, xo, xp, xn, ys, yo, yp, yn, out, pad; };
struct MsimMol { int off, n; };
struct MsimPair { int a, b, al_off, pad; };              // al_off: the pair's first atom in the overlaid copies

struct MsimIntArgs {
    const double *pos[3];             // (N, 3) of the three position sets
    const double *u[2], *v[2];        // per atom: alpha and p (shape), charge and nothing (esp)
    const double *cA, *cB;            // esp: (K)
    int K;
    const MsimJob *jobs;
    double *out;
};

struct MsimAlignArgs {
    const double *pos_a, *pos_b, *u[2], *v[2];
    const MsimMol *mol_a, *mol_b;
    const MsimPair *pairs;
    const int *list;                  // the pairs of this launch form
    int n_starts, max_iter;
    double gtol;
    const double *self;               // S_aa of every molecule of a, then S_bb of every molecule of b
    int n_mols_a;
    double *starts;                   // (P, n_starts, kMsimStartDoubles)
};

struct MsimFinishArgs {
    const MsimPair *pairs;
    const MsimMol *mol_a;
    int n_pairs, n_mols_a, n_mols_b, n_starts, metric, include_given;
    const double *integ;              // self a, self b, cross (P), and for an overlay with include_given the given pose's cross (P)
    const double *starts;
    const double *pos_a;
    double *out;                      // (P, 4): S_aa, S_bb, S_ab, score
    int *flags;                       // score: (P) zero denominator.  overlay: (P, 4) start, iterations, converged, zero denominator
    double *rot, *trans, *aligned;
};

#if defined(__HIPCC__) && !defined(SM_MOL_SIM_HOST_ONLY)

// v[0..NV) summed over the team in a fixed tree order; every thread gets the sums
template <int TEAM, int NV>
__device__ inline void msim_reduce(double *red, double *v) {
    const int t = threadIdx.x;
    __syncthreads();                                     // the call before has been read
#pragma unroll
    for (int k = 0; k < NV; ++k) red[k * TEAM + t] = v[k];
    __syncthreads();
    for (int s = TEAM / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < NV; ++k) red[k * TEAM + t] += red[k * TEAM + t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = red[k * TEAM];
}

// The sum over the atoms j of y (in LDS: x, y, z, u, v of TEAM entries each) for one atom of x; with GRAD also the derivative
// of the sum by the atom's position (shape mode).
template <int TEAM, int MODE, bool GRAD>
__device__ inline double msim_row(double px, double py, double pz, double ui, double vi, const double *sy, int ny, int K, const double *cA,
                                  const double *cB, double *g) {
    double f = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    for (int j = 0; j < ny; ++j) {
        const double dx = px - sy[j], dy = py - sy[TEAM + j], dz = pz - sy[2 * TEAM + j];
        const double r2 = (dx * dx + dy * dy) + dz * dz;
        if (MODE == MSIM_SHAPE) {
            const double uj = sy[3 * TEAM + j], s = ui + uj;
            const double A = (kMsimPi15 * (vi * sy[4 * TEAM + j])) / (s * sqrt(s)), B = (ui * uj) / s;
            const double term = A * exp(-(B * r2));
            f += term;
            if (GRAD) {
                const double c = (-2.0 * B) * term;
                gx += c * dx; gy += c * dy; gz += c * dz;
            }
        } else {
            double inner = 0.0;
            for (int k = 0; k < K; ++k) inner += cA[k] * exp(-(cB[k] * r2));
            f += inner * (ui * sy[3 * TEAM + j]);
        }
    }
    if (GRAD) { g[0] = gx; g[1] = gy; g[2] = gz; }
    return f;
}

template <int TEAM, int MODE>
__global__ __launch_bounds__(TEAM) void msim_integral_kernel(MsimIntArgs a) {
    __shared__ double s_y[5 * TEAM], s_red[TEAM];
    const MsimJob job = a.jobs[blockIdx.x];
    const int t = threadIdx.x;
    if (t < job.yn) {
        const double *p = a.pos[job.ys] + 3 * ((size_t)job.yo + t);
        s_y[t] = p[0]; s_y[TEAM + t] = p[1]; s_y[2 * TEAM + t] = p[2];
        s_y[3 * TEAM + t] = a.u[job.ys & 1][job.yp + t];
        s_y[4 * TEAM + t] = MODE == MSIM_SHAPE ? a.v[job.ys & 1][job.yp + t] : 0.0;
    }
    __syncthreads();
    double v[1] = {0.0};
    if (t < job.xn) {
        const double *p = a.pos[job.xs] + 3 * ((size_t)job.xo + t);
        const double ui = a.u[job.xs & 1][job.xp + t], vi = MODE == MSIM_SHAPE ? a.v[job.xs & 1][job.xp + t] : 0.0;
        v[0] = msim_row<TEAM, MODE, false>(p[0], p[1], p[2], ui, vi, s_y, job.yn, a.K, a.cA, a.cB, nullptr);
    }
    msim_reduce<TEAM, 1>(s_red, v);
    if (t == 0) a.out[job.out] = v[0];
}

// the score of a pair from its three integrals, as plain IEEE expressions; a zero denominator: NaN and the flag
__device__ inline double msim_metric(int metric, double saa, double sbb, double sab, int *flag) {
    const double den = metric == MSIM_CARBO ? sqrt(saa * sbb) : (saa + sbb) - sab;
    *flag = den == 0.0;
    return den == 0.0 ? __builtin_nan("") : sab / den;
}

__global__ __launch_bounds__(256) void msim_score_finish_kernel(MsimFinishArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n_pairs) return;
    const double saa = a.integ[a.pairs[p].a], sbb = a.integ[a.n_mols_a + a.pairs[p].b], sab = a.integ[a.n_mols_a + a.n_mols_b + p];
    int flag;
    const double score = msim_metric(a.metric, saa, sbb, sab, &flag);
    double *o = a.out + 4 * (size_t)p;
    o[0] = saa; o[1] = sbb; o[2] = sab; o[3] = score;
    a.flags[p] = flag;
}

// ---- the overlay ------------------------------------------------------------------------------------------------------------
// Eigenvectors of a symmetric 3x3 matrix by cyclic Jacobi rotations, columns ordered by ascending eigenvalue (ties: the
// earlier column first), the third replaced by the cross product of the first two: an orthonormal right-handed frame whatever
// the matrix (the identity for a zero matrix).  m: xx, yy, zz, xy, xz, yz.
__device__ inline void msim_frame(const double *m, double *V) {
    double A[3][3] = {{m[0], m[3], m[4]}, {m[3], m[1], m[5]}, {m[4], m[5], m[2]}};
    double E[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < kMsimSweeps; ++sweep) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int p = r == 2 ? 1 : 0, q = r == 0 ? 1 : 2;
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double x = A[k][p], y = A[k][q]; A[k][p] = c * x - s * y; A[k][q] = s * x + c * y; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double x = A[p][k], y = A[q][k]; A[p][k] = c * x - s * y; A[q][k] = s * x + c * y; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double x = E[k][p], y = E[k][q]; E[k][p] = c * x - s * y; E[k][q] = s * x + c * y; }
            A[p][q] = 0.0; A[q][p] = 0.0;
        }
    }
    const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
    // the columns of the smallest and of the middle eigenvalue
    int i0 = 0, i1 = 1;
    if (d1 < d0) { i0 = 1; i1 = 0; }
    const double e0 = i0 == 0 ? d0 : d1, e1 = i0 == 0 ? d1 : d0;
    if (d2 < e0) { i1 = i0; i0 = 2; } else if (d2 < e1) i1 = 2;
    double c0[3], c1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c0[k] = i0 == 0 ? E[k][0] : i0 == 1 ? E[k][1] : E[k][2];
        c1[k] = i1 == 0 ? E[k][0] : i1 == 1 ? E[k][1] : E[k][2];
    }
    V[0] = c0[0]; V[3] = c0[1]; V[6] = c0[2];
    V[1] = c1[0]; V[4] = c1[1]; V[7] = c1[2];
    V[2] = c0[1] * c1[2] - c0[2] * c1[1]; V[5] = c0[2] * c1[0] - c0[0] * c1[2]; V[8] = c0[0] * c1[1] - c0[1] * c1[0];
}

// R <- exp([w]x) R by Rodrigues' formula
__device__ inline void msim_rotate(const double *w, const double *R, double *out) {
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = sqrt(th2);
    double ka = 1.0, kb = 0.5;
    if (th > 1e-8) { ka = sin(th) / th; kb = (1.0 - cos(th)) / th2; }
    const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double Ex[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double w2 = (W[3 * r] * W[c] + W[3 * r + 1] * W[3 + c]) + W[3 * r + 2] * W[6 + c];
            Ex[3 * r + c] = ((r == c ? 1.0 : 0.0) + ka * W[3 * r + c]) + kb * w2;
        }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (Ex[3 * r] * R[c] + Ex[3 * r + 1] * R[3 + c]) + Ex[3 * r + 2] * R[6 + c];
}

// S_ab at the pose y_i = R a0_i + u and its derivative by (u, rotation about u): f and g (6)
template <int TEAM>
__device__ inline void msim_eval(const double *R, const double *u, bool own, const double *a0, double ui, double vi, const double *sb, int nb,
                                 double *red, double &f, double *g) {
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (own) {
        const double lx = (R[0] * a0[0] + R[1] * a0[1]) + R[2] * a0[2], ly = (R[3] * a0[0] + R[4] * a0[1]) + R[5] * a0[2],
                     lz = (R[6] * a0[0] + R[7] * a0[1]) + R[8] * a0[2];
        double fr[3];
        v[0] = msim_row<TEAM, MSIM_SHAPE, true>(lx + u[0], ly + u[1], lz + u[2], ui, vi, sb, nb, 0, nullptr, nullptr, fr);
        v[1] = fr[0]; v[2] = fr[1]; v[3] = fr[2];
        v[4] = ly * fr[2] - lz * fr[1]; v[5] = lz * fr[0] - lx * fr[2]; v[6] = lx * fr[1] - ly * fr[0];
    }
    msim_reduce<TEAM, 7>(red, v);
    f = v[0];
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = v[1 + k];
}

template <int TEAM>
__global__ __launch_bounds__(TEAM) void msim_align_kernel(MsimAlignArgs a) {
    __shared__ double s_b[5 * TEAM], s_red[7 * TEAM];
    const int t = threadIdx.x;
    const int p = a.list[blockIdx.x / a.n_starts], start = blockIdx.x % a.n_starts;
    const MsimPair pr = a.pairs[p];
    const MsimMol ma = a.mol_a[pr.a], mb = a.mol_b[pr.b];
    const bool own = t < ma.n, ownb = t < mb.n;
    double ax = 0.0, ay = 0.0, az = 0.0, ui = 1.0, vi = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
    if (own) {
        const double *q = a.pos_a + 3 * ((size_t)ma.off + t);
        ax = q[0]; ay = q[1]; az = q[2]; ui = a.u[0][ma.off + t]; vi = a.v[0][ma.off + t];
    }
    if (ownb) {
        const double *q = a.pos_b + 3 * ((size_t)mb.off + t);
        bx = q[0]; by = q[1]; bz = q[2];
        s_b[3 * TEAM + t] = a.u[1][mb.off + t]; s_b[4 * TEAM + t] = a.v[1][mb.off + t];
    }
    double c[6] = {ax, ay, az, bx, by, bz};
    msim_reduce<TEAM, 6>(s_red, c);
    const double ca[3] = {c[0] / ma.n, c[1] / ma.n, c[2] / ma.n}, cb[3] = {c[3] / mb.n, c[4] / mb.n, c[5] / mb.n};
    const double a0[3] = {own ? ax - ca[0] : 0.0, own ? ay - ca[1] : 0.0, own ? az - ca[2] : 0.0};
    const double b0[3] = {ownb ? bx - cb[0] : 0.0, ownb ? by - cb[1] : 0.0, ownb ? bz - cb[2] : 0.0};
    if (ownb) { s_b[t] = b0[0]; s_b[TEAM + t] = b0[1]; s_b[2 * TEAM + t] = b0[2]; }
    __syncthreads();                                     // b is staged before any thread sums over it
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, u[3] = {0.0, 0.0, 0.0};
    if (start < kMsimStarts) {
        // inertia tensors with unit weights about the centroids
        double ma6[6], mb6[6];
        {
            const double r2 = (a0[0] * a0[0] + a0[1] * a0[1]) + a0[2] * a0[2];
            ma6[0] = r2 - a0[0] * a0[0]; ma6[1] = r2 - a0[1] * a0[1]; ma6[2] = r2 - a0[2] * a0[2];
            ma6[3] = -(a0[0] * a0[1]); ma6[4] = -(a0[0] * a0[2]); ma6[5] = -(a0[1] * a0[2]);
            const double q2 = (b0[0] * b0[0] + b0[1] * b0[1]) + b0[2] * b0[2];
            mb6[0] = q2 - b0[0] * b0[0]; mb6[1] = q2 - b0[1] * b0[1]; mb6[2] = q2 - b0[2] * b0[2];
            mb6[3] = -(b0[0] * b0[1]); mb6[4] = -(b0[0] * b0[2]); mb6[5] = -(b0[1] * b0[2]);
        }
        msim_reduce<TEAM, 6>(s_red, ma6);
        msim_reduce<TEAM, 6>(s_red, mb6);
        double Va[9], Vb[9];
        msim_frame(ma6, Va);
        msim_frame(mb6, Vb);
        // R = Vb D Va^T, D = diag(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)
        const double d[3] = {start == 2 || start == 3 ? -1.0 : 1.0, start == 1 || start == 3 ? -1.0 : 1.0, start == 1 || start == 2 ? -1.0 : 1.0};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                R[3 * r + k] = (Vb[3 * r] * d[0] * Va[3 * k] + Vb[3 * r + 1] * d[1] * Va[3 * k + 1]) + Vb[3 * r + 2] * d[2] * Va[3 * k + 2];
    } else {
        u[0] = ca[0] - cb[0]; u[1] = ca[1] - cb[1]; u[2] = ca[2] - cb[2];
    }
    // BFGS on phi = -S_ab; every thread holds the same state and takes the same decisions
    const double scale = 0.5 * (a.self[pr.a] + a.self[a.n_mols_a + pr.b]), stop = a.gtol * scale;
    double f, g[6], H[36];
    msim_eval<TEAM>(R, u, own, a0, ui, vi, s_b, mb.n, s_red, f, g);
#pragma unroll
    for (int k = 0; k < 36; ++k) H[k] = k % 7 == 0 ? 1.0 : 0.0;
    bool scaled = false, identity = true;
    int it = 0, converged = 0;
    bool moved = false;
    while (true) {
        double gmax = 0.0;
        bool finite = f == f;                                  // fmax drops a NaN: test for it, a NaN pose is never converged
#pragma unroll
        for (int k = 0; k < 6; ++k) { gmax = fmax(gmax, fabs(g[k])); finite = finite && g[k] == g[k]; }
        if (!finite) break;
        if (gmax <= stop) { converged = 1; break; }
        if (it >= a.max_iter) break;
        ++it;
        // ascent direction d = H g (g is the gradient of S_ab = -grad phi)
        double d[6], gd = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) s += H[6 * r + k] * g[k];
            d[r] = s;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) gd += g[k] * d[k];
        if (!(gd > 0.0)) {                                     // not an ascent direction: steepest ascent
#pragma unroll
            for (int k = 0; k < 36; ++k) H[k] = k % 7 == 0 ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) d[k] = g[k];
            gd = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) gd += g[k] * g[k];
            scaled = false; identity = true;
        }
        double dmax = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) dmax = fmax(dmax, fabs(d[k]));
        if (dmax > kMsimStepMax) {
            const double sc = kMsimStepMax / dmax;
#pragma unroll
            for (int k = 0; k < 6; ++k) d[k] *= sc;
            gd *= sc;
        }
        double step = 1.0, fn = 0.0, gn[6], Rn[9], un[3], s6[6];
        bool accepted = false;
        for (int h = 0; h <= kMsimHalvings; ++h) {
#pragma unroll
            for (int k = 0; k < 6; ++k) s6[k] = step * d[k];
            un[0] = u[0] + s6[0]; un[1] = u[1] + s6[1]; un[2] = u[2] + s6[2];
            msim_rotate(s6 + 3, R, Rn);
            msim_eval<TEAM>(Rn, un, own, a0, ui, vi, s_b, mb.n, s_red, fn, gn);
            if (fn >= f + kMsimArmijo * step * gd) { accepted = true; break; }
            step *= 0.5;
        }
        if (!accepted) {
            if (identity) break;                               // steepest ascent found no increase: give up, not converged
#pragma unroll
            for (int k = 0; k < 36; ++k) H[k] = k % 7 == 0 ? 1.0 : 0.0;
            scaled = false; identity = true;
            continue;
        }
        // y = grad phi_new - grad phi = g - gn
        double y[6], sy = 0.0, yy = 0.0, ss = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) { y[k] = g[k] - gn[k]; sy += s6[k] * y[k]; yy += y[k] * y[k]; ss += s6[k] * s6[k]; }
        if (sy > 1e-10 * sqrt(ss * yy)) {
            if (!scaled) {
                const double h0 = sy / yy;
#pragma unroll
                for (int k = 0; k < 36; ++k) H[k] = k % 7 == 0 ? h0 : 0.0;
                scaled = true;
            }
            double Hy[6], yHy = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) s += H[6 * r + k] * y[k];
                Hy[r] = s;
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) yHy += y[k] * Hy[k];
            const double rho = 1.0 / sy, cs = (rho * rho) * yHy + rho;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int k = 0; k < 6; ++k) H[6 * r + k] = (H[6 * r + k] - rho * (s6[r] * Hy[k] + Hy[r] * s6[k])) + cs * (s6[r] * s6[k]);
            identity = false;
        }
        f = fn; moved = true;
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = gn[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
        u[0] = un[0]; u[1] = un[1]; u[2] = un[2];
    }
    if (t == 0) {
        double *o = a.starts + ((size_t)p * a.n_starts + start) * kMsimStartDoubles;
        o[0] = f;
        if (start == kMsimStarts && !moved) {                  // the pose as given, kept: the identity, exactly
            for (int k = 0; k < 9; ++k) o[1 + k] = k % 4 == 0 ? 1.0 : 0.0;
            o[10] = 0.0; o[11] = 0.0; o[12] = 0.0;
        } else {
            for (int k = 0; k < 9; ++k) o[1 + k] = R[k];
            // x' = R (x - ca) + u + cb = R x + t
            for (int r = 0; r < 3; ++r) o[10 + r] = (u[r] + cb[r]) - ((R[3 * r] * ca[0] + R[3 * r + 1] * ca[1]) + R[3 * r + 2] * ca[2]);
        }
        o[13] = (double)it; o[14] = (double)converged; o[15] = moved ? 1.0 : 0.0;
    }
}

__device__ inline void msim_apply(const double *R, const double *tr, const double *x, double *o) {
    o[0] = ((R[0] * x[0] + R[1] * x[1]) + R[2] * x[2]) + tr[0];
    o[1] = ((R[3] * x[0] + R[4] * x[1]) + R[5] * x[2]) + tr[1];
    o[2] = ((R[6] * x[0] + R[7] * x[1]) + R[8] * x[2]) + tr[2];
}

// per pair: the start with the largest S_ab (ties: the lowest index; NaN never wins), its motion, and the moved copy of a
__global__ __launch_bounds__(64) void msim_pick_kernel(MsimFinishArgs a) {
    const int p = blockIdx.x;
    const MsimPair pr = a.pairs[p];
    const MsimMol ma = a.mol_a[pr.a];
    const double *st = a.starts + (size_t)p * a.n_starts * kMsimStartDoubles;
    int best = 0;
    for (int s = 1; s < a.n_starts; ++s) {
        const double fb = st[best * kMsimStartDoubles], fs = st[s * kMsimStartDoubles];
        if (fs > fb || (fb != fb && fs == fs)) best = s;
    }
    const double *o = st + best * kMsimStartDoubles;
    if (threadIdx.x == 0) {
        for (int k = 0; k < 9; ++k) a.rot[9 * (size_t)p + k] = o[1 + k];
        for (int k = 0; k < 3; ++k) a.trans[3 * (size_t)p + k] = o[10 + k];
        int *info = a.flags + 4 * (size_t)p;
        info[0] = best; info[1] = (int)o[13]; info[2] = (int)o[14]; info[3] = 0;
    }
    for (int i = threadIdx.x; i < ma.n; i += 64)
        msim_apply(o + 1, o + 10, a.pos_a + 3 * ((size_t)ma.off + i), a.aligned + 3 * ((size_t)pr.al_off + i));
}

// per pair: the score of the overlaid copy; with include_given the pose as given replaces it when it scores higher
__global__ __launch_bounds__(64) void msim_align_finish_kernel(MsimFinishArgs a) {
    const int p = blockIdx.x;
    const MsimPair pr = a.pairs[p];
    const MsimMol ma = a.mol_a[pr.a];
    const double saa = a.integ[pr.a], sbb = a.integ[a.n_mols_a + pr.b];
    double sab = a.integ[a.n_mols_a + a.n_mols_b + p];
    bool given = false;
    if (a.include_given) {
        const double sg = a.integ[a.n_mols_a + a.n_mols_b + a.n_pairs + p];
        given = sg > sab || (sab != sab && sg == sg);
        if (given) sab = sg;
    }
    if (given)
        for (int i = threadIdx.x; i < ma.n; i += 64) {
            const double *x = a.pos_a + 3 * ((size_t)ma.off + i);
            double *o = a.aligned + 3 * ((size_t)pr.al_off + i);
            o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
        }
    if (threadIdx.x == 0) {
        int *info = a.flags + 4 * (size_t)p, flag;
        const double score = msim_metric(MSIM_TANIMOTO, saa, sbb, sab, &flag);
        double *o = a.out + 4 * (size_t)p;
        o[0] = saa; o[1] = sbb; o[2] = sab; o[3] = score;
        info[3] = flag;
        if (given) {
            const double *st = a.starts + ((size_t)p * a.n_starts + kMsimStarts) * kMsimStartDoubles;
            for (int k = 0; k < 9; ++k) a.rot[9 * (size_t)p + k] = k % 4 == 0 ? 1.0 : 0.0;
            for (int k = 0; k < 3; ++k) a.trans[3 * (size_t)p + k] = 0.0;
            // the flag of the pose returned: start 4's own when it never left that pose, else 0 (the pose as given is then
            // not where the optimiser stopped, and nothing says it is stationary)
            info[0] = kMsimStarts; info[1] = 0; info[2] = st[15] == 0.0 ? (int)st[14] : 0;
        }
    }
}

#endif  // device code

// ---- host plan --------------------------------------------------------------------------------------------------------------
struct MsimSet { int64_t n_mols; const int64_t *off; const double *u, *v; };      // host views; v: null in esp mode

struct MsimPlan {
    std::vector<MsimMol> mol[2];
    std::vector<MsimPair> pairs;
    std::vector<int> form;            // per pair: 0 wave, 1 block
    std::vector<int> list[2];         // the pairs of each form
    int64_t n_atoms[2] = {0, 0}, n_aligned = 0;
};

inline int msim_form(int na, int nb) { return std::max(na, nb) > kMsimWaveAtoms; }

inline std::string msim_set_error(int mode, const char *name, const MsimSet &s, std::vector<MsimMol> &mol, int64_t &n_atoms) {
    const std::string who = std::string("molecule similarity: set ") + name;
    if (s.n_mols < 1 || s.n_mols > kMsimMaxMols || !s.off) return who + " needs 1.." + std::to_string(kMsimMaxMols) + " molecules, got " + std::to_string(s.n_mols);
    if (!s.u || (mode == MSIM_SHAPE && !s.v)) return who + " lacks its per-atom parameters";
    if (s.off[0] != 0) return who + ": the offsets must start at 0";
    mol.resize((size_t)s.n_mols);
    for (int64_t m = 0; m < s.n_mols; ++m) {
        const int64_t n = s.off[m + 1] - s.off[m];
        if (n < 1) return who + ": molecule " + std::to_string(m) + " has no atoms";
        if (n > kMsimMaxAtoms) return who + ": molecule " + std::to_string(m) + " has " + std::to_string(n) + " atoms; the limit is " + std::to_string(kMsimMaxAtoms);
        mol[(size_t)m] = {(int)s.off[m], (int)n};
    }
    n_atoms = s.off[s.n_mols];
    for (int64_t i = 0; i < n_atoms; ++i) {
        if (mode == MSIM_SHAPE) {
            if (!std::isfinite(s.u[i]) || !(s.u[i] > 0.0)) return who + ": atom " + std::to_string(i) + " has a Gaussian width that is not finite and positive";
            if (!std::isfinite(s.v[i])) return who + ": atom " + std::to_string(i) + " has a prefactor that is not finite";
        } else if (!std::isfinite(s.u[i])) return who + ": atom " + std::to_string(i) + " has a charge that is not finite";
    }
    return "";
}

// Checks a call and lays out its pairs.  "" or the refusal's message; `out` may be null.
inline std::string msim_plan(int mode, const MsimSet &a, const MsimSet &b, int64_t n_pairs, const int64_t *pairs, int n_terms, const double *cA,
                             const double *cB, MsimPlan *out) {
    if (mode != MSIM_SHAPE && mode != MSIM_ESP) return "molecule similarity: unknown mode " + std::to_string(mode);
    if (mode == MSIM_ESP) {
        if (n_terms < 1 || n_terms > kMsimMaxTerms || !cA || !cB) return "molecule similarity: 1.." + std::to_string(kMsimMaxTerms) + " Gaussian terms, got " + std::to_string(n_terms);
        for (int k = 0; k < n_terms; ++k)
            if (!std::isfinite(cA[k]) || !std::isfinite(cB[k])) return "molecule similarity: term " + std::to_string(k) + " has a coefficient that is not finite";
    }
    MsimPlan pl;
    std::string e = msim_set_error(mode, "a", a, pl.mol[0], pl.n_atoms[0]);
    if (e.empty()) e = msim_set_error(mode, "b", b, pl.mol[1], pl.n_atoms[1]);
    if (!e.empty()) return e;
    if (n_pairs < 1 || n_pairs > kMsimMaxPairs || !pairs) return "molecule similarity: 1.." + std::to_string(kMsimMaxPairs) + " pairs, got " + std::to_string(n_pairs);
    pl.pairs.resize((size_t)n_pairs); pl.form.resize((size_t)n_pairs);
    int64_t al = 0;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t ia = pairs[2 * p], ib = pairs[2 * p + 1];
        if (ia < 0 || ia >= a.n_mols) return "molecule similarity: pair " + std::to_string(p) + " names molecule " + std::to_string(ia) + " of set a, which has " + std::to_string(a.n_mols);
        if (ib < 0 || ib >= b.n_mols) return "molecule similarity: pair " + std::to_string(p) + " names molecule " + std::to_string(ib) + " of set b, which has " + std::to_string(b.n_mols);
        if (al > (1ll << 30)) return "molecule similarity: the pairs' first molecules have more than 2^30 atoms together";
        pl.pairs[(size_t)p] = {(int)ia, (int)ib, (int)al, 0};
        const int form = msim_form(pl.mol[0][(size_t)ia].n, pl.mol[1][(size_t)ib].n);
        pl.form[(size_t)p] = form;
        pl.list[form].push_back((int)p);
        al += pl.mol[0][(size_t)ia].n;
    }
    pl.n_aligned = al;
    if (out) *out = std::move(pl);
    return "";
}

// The integrals of a call as jobs by form.  Slots: self a (M_a), self b (M_b), then per pair the cross integral of
// position set `xs` (0: a as given, 2: the overlaid copies) at slot_base + p.
inline void msim_self_jobs(const MsimPlan &pl, std::vector<MsimJob> (&jobs)[2]) {
    int slot = 0;
    for (int s = 0; s < 2; ++s)
        for (const MsimMol &m : pl.mol[s]) jobs[msim_form(m.n, m.n)].push_back({s, m.off, m.off, m.n, s, m.off, m.off, m.n, slot++, 0});
}

inline void msim_cross_jobs(const MsimPlan &pl, int xs, int slot_base, std::vector<MsimJob> (&jobs)[2]) {
    for (size_t p = 0; p < pl.pairs.size(); ++p) {
        const MsimMol &ma = pl.mol[0][(size_t)pl.pairs[p].a], &mb = pl.mol[1][(size_t)pl.pairs[p].b];
        jobs[pl.form[p]].push_back({xs, xs == 2 ? pl.pairs[p].al_off : ma.off, ma.off, ma.n, 1, mb.off, mb.off, mb.n, slot_base + (int)p, 0});
    }
}
