// Workgroup-level (256 threads) dense K x K stages of the precision draws (precision.hip): the shifted load
// I + scale * M, the in-place Gauss-Jordan inverse with its log det, and the product of the inverse with a
// block of columns.  A header of their own so that tests/kunit/kunit.hip calls the product's text.
#pragma once
#include "handoff.h"
#include "linalg.h"

namespace dcfm {

constexpr int PREC_PANEL = 16;    // right-hand columns of a product staged in LDS

// A (N x N, LDS) = I + scale * src (N x N of a global matrix with rows ld apart, agent-scope), eight loads in
// flight per thread
__device__ __forceinline__ void load_shifted(double *A, int N, const double *src, int ld, double scale) {
    constexpr int FU = 8;
    for (int e0 = threadIdx.x; e0 < N * N; e0 += 256 * FU) {
        double v[FU];
        int i[FU], j[FU];
#pragma unroll
        for (int u = 0; u < FU; ++u) {
            const int e = min(e0 + 256 * u, N * N - 1);
            i[u] = e / N;
            j[u] = e - i[u] * N;
            v[u] = ld_agent(src + (size_t)i[u] * ld + j[u]);
        }
#pragma unroll
        for (int u = 0; u < FU; ++u)
            if (e0 + 256 * u < N * N) A[i[u] * N + j[u]] = fma(scale, v[u], i[u] == j[u] ? 1.0 : 0.0);
    }
}

// A (N x N in LDS, row-major, SPD) := A^{-1} in place by Gauss-Jordan elimination on the pivots in index
// order, GJ_B = 4 at a time, every entry updated by the operations of the unblocked sweep in its order.
// Every thread eliminates the 4 x 4 pivot block in registers and runs its own column of the pivot rows
// (a unit vector for a column of the block) through the same eliminations: R is the column of the
// finished pivot rows, U[q] its entry in pivot row q as that row stands when pivot q is taken, S[q][c]
// that row's entry in the block's later column c.  A row i outside the block needs its multipliers
// m_q = A(i, blk_q) - sum_{q' < q} m_q' S[q'][q], formed once per row into Cc (N x 4 doubles, 16-byte
// aligned), and then A(i, j) -= sum_q m_q U[q]: one read and one write of A per four pivots and two
// barriers (one pivot at a time, the LDS traffic of the rank-1 updates and the per-pivot latency chain
// made a K = 100 inversion 400 us).  The product of the panel with the finished rows R
// instead would be the same in exact arithmetic but loses cond(block) on the way.  A last
// block of fewer than four pivots is padded with an identity.  Returns log det A, the sum of the
// pivots' logs (the same value in every thread).  256 threads; ceil(N / 4) passes of fixed length
// whatever the data
constexpr int GJ_B = 4;
__device__ __forceinline__ double gj_invert(double *A, int N, double *Cc) {
    const int t = threadIdx.x;
    const int nj = N <= 32 ? 32 : (N <= 64 ? 64 : 128), j = t & (nj - 1), i0 = t / nj, di = 256 / nj;
    double lg = 0.0;
    __syncthreads();
#pragma unroll 1
    for (int kb = 0; kb < N; kb += GJ_B) {
        const int bs = min(GJ_B, N - kb);
        double Pm[GJ_B][GJ_B];
#pragma unroll
        for (int r = 0; r < GJ_B; ++r)
#pragma unroll
            for (int c = 0; c < GJ_B; ++c)
                Pm[r][c] = r < bs && c < bs ? A[(kb + r) * N + kb + c] : (r == c ? 1.0 : 0.0);
        const bool jin = j >= kb && j < kb + bs;          // a column of the pivot block: its panel entries are I
        double R[GJ_B], U[GJ_B], S[GJ_B][GJ_B];
#pragma unroll
        for (int c = 0; c < GJ_B; ++c)
            R[c] = c < bs && j < N ? (jin ? (j - kb == c ? 1.0 : 0.0) : A[(kb + c) * N + j]) : 0.0;
#pragma unroll
        for (int q = 0; q < GJ_B; ++q) {
            const double piv = Pm[q][q];
            lg += log(piv);
            const double ip = 1.0 / piv;
            double rq[GJ_B];
#pragma unroll
            for (int c = 0; c < GJ_B; ++c) rq[c] = (c == q ? 1.0 : Pm[q][c]) * ip;
            const double aq = R[q] * ip;
#pragma unroll
            for (int r = 0; r < GJ_B; ++r) {
                if (r == q) continue;
                const double f = Pm[r][q];
#pragma unroll
                for (int c = 0; c < GJ_B; ++c) Pm[r][c] = fma(-f, rq[c], c == q ? 0.0 : Pm[r][c]);
                R[r] = fma(-f, aq, R[r]);
            }
#pragma unroll
            for (int c = 0; c < GJ_B; ++c) {
                Pm[q][c] = rq[c];
                S[q][c] = rq[c];
            }
            R[q] = aq;
            U[q] = aq;
        }
        for (int i = t; i < N; i += 256) {                // the multipliers of row i (0 for a row of the block)
            const bool out = !(i >= kb && i < kb + bs);
            double m[GJ_B];
#pragma unroll
            for (int c = 0; c < GJ_B; ++c) m[c] = c < bs && out ? A[i * N + kb + c] : 0.0;
#pragma unroll
            for (int q = 0; q < GJ_B; ++q)
#pragma unroll
                for (int c = q + 1; c < GJ_B; ++c) m[c] = fma(-m[q], S[q][c], m[c]);
#pragma unroll
            for (int c = 0; c < GJ_B; ++c) Cc[i * GJ_B + c] = m[c];
        }
        __syncthreads();
        if (j < N) {   // eight rows of the column at a time: the LDS reads go out before the first FMA waits
            constexpr int FU = 8;
            for (int ib = i0; ib < N; ib += FU * di) {
                double a[FU];
                d2 c01[FU], c23[FU];
#pragma unroll
                for (int u = 0; u < FU; ++u) {
                    const int i = min(ib + u * di, N - 1);
                    a[u] = A[i * N + j];
                    c01[u] = *reinterpret_cast<const d2 *>(Cc + i * GJ_B);
                    c23[u] = *reinterpret_cast<const d2 *>(Cc + i * GJ_B + 2);
                }
#pragma unroll
                for (int u = 0; u < FU; ++u) {
                    const int i = ib + u * di, d = i - kb;
                    if (i >= N) continue;
                    double v = jin ? 0.0 : a[u];
                    v = fma(-c01[u][0], U[0], v);
                    v = fma(-c01[u][1], U[1], v);
                    v = fma(-c23[u][0], U[2], v);
                    v = fma(-c23[u][1], U[3], v);
                    if (d >= 0 && d < bs) v = d == 0 ? R[0] : (d == 1 ? R[1] : (d == 2 ? R[2] : R[3]));
                    A[i * N + j] = v;
                }
            }
        }
        __syncthreads();
    }
    return lg;
}

// dst (N x ncols, ldd) = A (N x N, LDS) times src (N x ncols, lds_, global), PREC_PANEL columns at a time
// through sP; src is read and dst written agent-scope
__device__ __forceinline__ void mat_apply(const double *A, int N, const double *src, int lds_, int ncols, double *dst,
                                          int ldd, double *sP) {
    const int t = threadIdx.x, cc = t & (PREC_PANEL - 1);
    for (int c0 = 0; c0 < ncols; c0 += PREC_PANEL) {
        for (int e = t; e < N * PREC_PANEL; e += 256) {
            const int c = c0 + (e & (PREC_PANEL - 1));
            sP[e] = c < ncols ? ld_agent(src + (size_t)(e / PREC_PANEL) * lds_ + c) : 0.0;
        }
        __syncthreads();
        // a thread's rows t / 16 + 16 u of column cc: N <= 128 gives at most 8, independent accumulators
        constexpr int NU = KP_MAX * PREC_PANEL / 256;
        const int ib = t / PREC_PANEL;
        double acc[NU];
        int ro[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            acc[u] = 0.0;
            ro[u] = min(ib + (256 / PREC_PANEL) * u, N - 1) * N;
        }
#pragma unroll 2
        for (int j = 0; j < N; ++j) {
            const double b = sP[j * PREC_PANEL + cc];
#pragma unroll
            for (int u = 0; u < NU; ++u) acc[u] = fma(A[ro[u] + j], b, acc[u]);
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = ib + (256 / PREC_PANEL) * u;
            if (i < N && c0 + cc < ncols) st_agent(dst + (size_t)i * ldd + c0 + cc, acc[u]);
        }
        __syncthreads();
    }
}

}  // namespace dcfm
