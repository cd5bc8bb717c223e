// Y = Sigmaout V for a block of up to 32 right-hand sides, on the device (dcfm_sigma_apply).
//
// Sigmaout is the lower triangle in 128 x 128 tiles, each stored as k_assemble's accumulators
// (sig_tile_off: the f64 MFMA C/D image of its 16 x 16 sub-tiles).  A stored tile T = (ti, tj) is
// read ONCE and used twice:
//     Y[rows of ti] += T  V[rows of tj]        (P1)
//     Y[rows of tj] += T' V[rows of ti]        (P2, off-diagonal tiles)
// The diagonal tile holds authoritative values only for a >= b: P1 takes its lower triangle with
// the diagonal, P2 the strict lower triangle, which together are the mirrored tile.  Rows >= p of
// a partial tile are masked by a select (never a product with zero), so nothing stored there can
// reach Y.
//
// Operand layouts (v_mfma_f64_16x16x4_f64: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4]
// [j = lane & 15], C/D row = (lane >> 4) + 4 reg, col = lane & 15).  Register g of a loaded
// sub-tile is, lane by lane, T[4 g + (lane >> 4)][lane & 15]: read as an A operand its i index runs
// over T's COLUMNS and its k index over the rows 4 g .. 4 g + 3.  So the stored image feeds the
// transposed product P2 directly (one MFMA per g, contraction over the sub-tile's rows), and
// the plain product P1 needs T[row = lane & 15][col = 4 s + (lane >> 4)]: a transpose, done per
// sub-tile through a wave-private 16 x 17 LDS pad.
//
// Block = 4 waves = one strip of up to APPLY_STRIP tiles of tile row ti.  Wave w owns the tile
// columns [32 w, 32 w + 32) over all 128 rows (any wave can read any (u, v, h) slice: 1 KiB
// contiguous), so P2 -- indexed by tile column -- is complete inside the wave and goes straight to
// the tile's partial panel.  P1 -- indexed by tile row -- stays in the wave's accumulators across
// the strip (V's panel for the rows of ti is staged once per strip) and the four waves' column
// shares are added through LDS in wave order at the end of the strip.
//
// Deterministic: no atomics.  P1 partials [tile row][strip], P2 partials [tile]; k_sigma_apply_sum
// adds, for every output row, the strips of its tile row in strip order and then the tiles of its
// tile column in row order.
//
// Traffic per block of vectors: the stored triangle once (4 p^2 bytes) plus the P2 panels written
// and read once, (nvp / 128) of that each (nvp = 16 or 32 padded right-hand sides).
#include <hip/hip_runtime.h>

#include "dcfm_internal.h"
#include "linalg.h"

#include <algorithm>

namespace dcfm {

constexpr int APPLY_STRIP = 8;    // tiles of one tile row per block
constexpr int APPLY_TP = 17;      // pitch of the transposition pad

// V's rows [row0, row0 + 128) (p x nv column-major, leading dimension p) into X[cg][row][16],
// zero-padded to 128 rows and 16 NC columns
template <int NC>
__device__ __forceinline__ void stage_panel(const double *__restrict__ V, int p, int nv, int row0,
                                            double (*X)[ASM_TILE][16]) {
    for (int e = threadIdx.x; e < ASM_TILE * 16 * NC; e += 256) {
        const int row = e & (ASM_TILE - 1), c = e >> 7;
        const int a = row0 + row;
        X[c >> 4][row][c & 15] = (a < p && c < nv) ? V[(size_t)c * p + a] : 0.0;
    }
}

template <int NC>
__global__ __launch_bounds__(256) void k_sigma_apply(const double *__restrict__ S, int p, int T0, int T1,
                                                     const double *__restrict__ V, int nv,
                                                     double *__restrict__ P1, double *__restrict__ P2,
                                                     int nstrip) {
    constexpr int NVP = 16 * NC;
    const int ti = T0 + blockIdx.y, strip = blockIdx.x;
    const int tj0 = strip * APPLY_STRIP;
    if (ti >= T1 || tj0 > ti) return;
    const int tj1 = min(ti + 1, tj0 + APPLY_STRIP);
    __shared__ double Xi[NC][ASM_TILE][16];       // V rows of ti; at the end of the strip: the P1 reduction
    __shared__ double Xj[NC][ASM_TILE][16];       // V rows of tj
    __shared__ double pad[4][16][APPLY_TP];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int r = lane & 15, q = lane >> 4;
    volatile double(*tp)[APPLY_TP] = pad[wave];

    stage_panel<NC>(V, p, nv, ti * ASM_TILE, Xi);
    d4 acc1[8][NC];
#pragma unroll
    for (int R = 0; R < 8; ++R)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc1[R][c] = d4{0.0, 0.0, 0.0, 0.0};

    for (int tj = tj0; tj < tj1; ++tj) {
        const bool diag = tj == ti;
        const double *__restrict__ St = S + (size_t)(tri(ti) - tri(T0) + tj) * ASM_TILE * ASM_TILE;
        __syncthreads();                           // the previous tile's Xj reads are done
        stage_panel<NC>(V, p, nv, tj * ASM_TILE, Xj);
        __syncthreads();
        d4 acc2[2][NC];
#pragma unroll
        for (int vv = 0; vv < 2; ++vv)
#pragma unroll
            for (int c = 0; c < NC; ++c) acc2[vv][c] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int R = 0; R < 8; ++R) {              // 16-row block R of the tile
            const int quad = 2 * (R >> 2) + (wave >> 1), u = R & 3;
            double x[2][4];
#pragma unroll
            for (int vv = 0; vv < 2; ++vv)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const d2 o = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(
                        St + sig_tile_off(u, 2 * (wave & 1) + vv, 2 * h, quad, lane)));
                    x[vv][2 * h] = o.x;
                    x[vv][2 * h + 1] = o.y;
                }
#pragma unroll
            for (int vv = 0; vv < 2; ++vv) {
                const int cb = 32 * wave + 16 * vv;          // first tile column of the sub-tile
                double lo[4];                                // a >= b (P1)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ra = 16 * R + q + 4 * g, a = ti * ASM_TILE + ra;
                    const bool live = a < p;
                    lo[g] = (live && (!diag || ra >= cb + r)) ? x[vv][g] : 0.0;
                    const double st = (live && (!diag || ra > cb + r)) ? x[vv][g] : 0.0;   // a > b (P2)
                    // P2: A = the stored image, k = the rows 4 g .. 4 g + 3 of block R
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                        acc2[vv][c] = mfma16x16x4(st, Xi[c][16 * R + 4 * g + q][r], acc2[vv][c]);
                }
                // P1: the sub-tile transposed through the wave's pad
#pragma unroll
                for (int g = 0; g < 4; ++g) tp[q + 4 * g][r] = lo[g];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const double a1 = tp[r][4 * s + q];
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                        acc1[R][c] = mfma16x16x4(a1, Xj[c][cb + 4 * s + q][r], acc1[R][c]);
                }
            }
        }
        // the tile's P2 panel: rows = the tile's columns, [128][NVP]
        double *__restrict__ o2 = P2 + (size_t)(tri(ti) - tri(T0) + tj) * ASM_TILE * NVP;
#pragma unroll
        for (int vv = 0; vv < 2; ++vv)
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    o2[(size_t)(32 * wave + 16 * vv + q + 4 * g) * NVP + 16 * c + r] = acc2[vv][c][g];
    }
    // P1 of the strip: the waves' column shares added in wave order
    double *red = &Xi[0][0][0];                    // [128][NVP]
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int R = 0; R < 8; ++R)
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        double *d = red + (16 * R + q + 4 * g) * NVP + 16 * c + r;
                        *d = (w == 0) ? acc1[R][c][g] : *d + acc1[R][c][g];
                    }
        }
    }
    __syncthreads();
    double *__restrict__ o1 = P1 + ((size_t)blockIdx.y * nstrip + strip) * ASM_TILE * NVP;
    for (int e = t; e < ASM_TILE * NVP; e += 256) o1[e] = red[e];
}

// Y[a][c] (p x nv column-major) = the P1 strips of a's tile row in strip order, then the P2 panels of
// a's tile column in tile-row order; only this rank's tile rows [T0, T1)
__global__ __launch_bounds__(256) void k_sigma_apply_sum(const double *__restrict__ P1,
                                                         const double *__restrict__ P2, int p, int T0, int T1,
                                                         int nvp, int nv, int nstrip, double *__restrict__ Y) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)p * nvp) return;
    const int c = (int)(e % nvp), a = (int)(e / nvp);
    if (c >= nv) return;
    const int tt = a / ASM_TILE, i = a % ASM_TILE;
    double acc = 0.0;
    if (tt >= T0 && tt < T1) {
        const int ns = tt / APPLY_STRIP + 1;
        for (int s = 0; s < ns; ++s) acc += P1[(((size_t)(tt - T0) * nstrip + s) * ASM_TILE + i) * nvp + c];
    }
    for (int ti = max(tt, T0); ti < T1; ++ti)
        acc += P2[((size_t)(tri(ti) - tri(T0) + tt) * ASM_TILE + i) * nvp + c];
    Y[(size_t)c * p + a] = acc;
}

int sigma_apply_width(int nv) { return nv <= 16 ? 16 : 32; }
int sigma_apply_strips(int T1) { return cdiv(std::max(T1, 1), APPLY_STRIP); }
size_t sigma_apply_scratch(int T0, int T1, int nv) {
    const size_t nvp = (size_t)sigma_apply_width(nv);
    return ((size_t)std::max(T1 - T0, 0) * sigma_apply_strips(T1) + (size_t)(tri(T1) - tri(T0))) * ASM_TILE * nvp;
}
void launch_sigma_apply(const double *S, int p, int T0, int T1, const double *V, int nv, double *scratch, double *Y,
                        hipStream_t s) {
    const int nvp = sigma_apply_width(nv), nstrip = sigma_apply_strips(T1);
    double *P1 = scratch, *P2 = scratch + (size_t)std::max(T1 - T0, 0) * nstrip * ASM_TILE * nvp;
    if (T1 > T0) {
        const dim3 grid(nstrip, T1 - T0);
        if (nvp == 16) hipLaunchKernelGGL(k_sigma_apply<1>, grid, dim3(256), 0, s, S, p, T0, T1, V, nv, P1, P2, nstrip);
        else hipLaunchKernelGGL(k_sigma_apply<2>, grid, dim3(256), 0, s, S, p, T0, T1, V, nv, P1, P2, nstrip);
    }
    const size_t tot = (size_t)p * nvp;
    hipLaunchKernelGGL(k_sigma_apply_sum, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, P1, P2, p, T0, T1, nvp,
                       nv, nstrip, Y);
}

}  // namespace dcfm
