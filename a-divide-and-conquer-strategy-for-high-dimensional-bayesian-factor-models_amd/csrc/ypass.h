// The two passes over Y of one iteration, fp64 MFMA, templated on the padded factor width KW:
//   pass 1 (k_wpass, k_wcol's W tiles)  W_m = Y_m (w o Lambda_m)                       dc:101,121
//   pass 2 (k_cpass)                    [C_m | E_m] = [Y_m | eta_m]' eta_m             dc:133,138,141
#pragma once
#include "dcfm_internal.h"
#include "linalg.h"

namespace dcfm {

#ifndef DCFM_WP_RING
#define DCFM_WP_RING 3
#endif
constexpr int WP_RING = DCFM_WP_RING;   // W pass register ring depth (chunks)
#ifndef DCFM_WP_RING_WIDE
#define DCFM_WP_RING_WIDE 4
#endif
// the wide layouts' pass (k_wpass<64 / 128>: 2 waves per SIMD at c4) takes one chunk more in flight
// (c4: 152 -> 127 us; ab_rg in profiles/r06_ab_summary.txt); the same products in the same order
constexpr int WP_RING_WIDE = DCFM_WP_RING_WIDE;
#ifndef DCFM_WP_SKIP_PAD
#define DCFM_WP_SKIP_PAD 1
#endif
constexpr bool WP_SKIP_PAD = DCFM_WP_SKIP_PAD;   // 0: the A/B baseline, every chunk of PP (wpass_acc)
// ============================================================================
// W pass: W_m[i][k] = sum_j Y_m[i][j] (w_j Lambda_m[j][k])   fp64 MFMA, Y pass 1
// one wave = (shard m, 16 MT rows i = MT M-tiles) x 32 k (even / odd k tiles) of
// column tile kt (KW/32 tiles, adjacent in the 1-D grid so the wide layouts re-read Y from L2),
// reduction over j in chunks of 8: lane (r, q) holds Y[i0+r][8t+2q .. +1] (16 B);
// k-step 2t uses element 0, 2t+1 element 1; the (w_j L[j][2r], w_j L[j][2r+1]) values use the
// same j <-> (q, e) map.  The product is formed transposed, W' = (w o L)' Y' (the Lambda values
// the A operand, Y the B operand: the same products in the same order per element), so lane
// (r, q) ends with W[i0 + 16a + r][8g + 2q + tb] in acc[a][tb][g] — row = lane & 15, the layout
// the Z draw takes its W operand in (zdraw_rows; k_wcol draws Z from these registers).
// MT = 1 (64-row blocks, twice the blocks) where the launch would not fill the chip (a few
// shards per rank): each element's reduction order is the same for both, so the choice
// changes no bit of W.
// ============================================================================
// Register ring of R chunks (WP_RING; WP_RING_WIDE for KW > 32): chunk t + R - 1 is requested
// while chunk t multiplies, so R - 1 chunks are in flight behind the MFMAs.  pre() runs once the
// first R - 1 chunks' loads are issued (VALU work hidden behind their latency).
template <int KW, int MT, int R = (KW > KP ? WP_RING_WIDE : WP_RING), class Pre>
__device__ __forceinline__ void wpass_acc(const Dims &d, const double *__restrict__ Y, const double *__restrict__ Lam,
                                          const double *__restrict__ omega, int m, int i0, int kt, d4 (&acc)[MT][2],
                                          Pre &&pre) {
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const double *Y0 = Y + ((size_t)m * d.NP + i0 + r) * d.PP + 2 * q;
    const double *Y1 = Y0 + (size_t)16 * (MT - 1) * d.PP;
    const double *L = Lam + (size_t)m * d.PP * KW + 32 * kt + 2 * r;
    const double *wp = omega + (size_t)m * d.PP + 2 * q;
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
    // The reduction stops at the last chunk that holds a data column, ceil(P / 8), not at PP / 8: Y's
    // padding columns j >= P are zeros (dcfm_set_data, k_stdize), so every product of a whole padding
    // chunk is +-0 whatever omega and Lambda hold there, and an accumulator that starts at +0 and only
    // ever adds is never -0, hence unchanged by adding them (c3: P = 312, PP = 320, chunk 39 of 40).
    // A last partial chunk stays: its padding columns are those zeros of Y.  No caller reads past the
    // accumulators (wpass_tile's stores and k_wcol's Z draw take acc alone), so none relies on the
    // padded chunks.  The residual kernels reduce over the rows i, not over j: nothing to skip there.
    const int nch = WP_SKIP_PAD ? (d.P + 7) >> 3 : d.PP >> 3;
    d2 y0[R], y1[R], ww[R], l0[R], l1[R];
    auto load = [&](int t, int k) {
        const int j = 8 * t;
        y0[k] = *reinterpret_cast<const d2 *>(Y0 + j);
        if (MT == 2) y1[k] = *reinterpret_cast<const d2 *>(Y1 + j);
        ww[k] = *reinterpret_cast<const d2 *>(wp + j);
        l0[k] = *reinterpret_cast<const d2 *>(L + (size_t)(j + 2 * q) * KW);
        l1[k] = *reinterpret_cast<const d2 *>(L + (size_t)(j + 2 * q + 1) * KW);
    };
    // the two k-steps of a chunk accumulate into separate sets (8 independent MFMA chains per wave
    // instead of 4), added at the end: W = (sum over even j) + (sum over odd j)
    d4 acc2[MT][2];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc2[a][b] = d4{0.0, 0.0, 0.0, 0.0};
    auto mma = [&](int k) {
        const double b00 = ww[k].x * l0[k].x, b01 = ww[k].x * l0[k].y;
        const double b10 = ww[k].y * l1[k].x, b11 = ww[k].y * l1[k].y;
        acc[0][0] = mfma16x16x4(b00, y0[k].x, acc[0][0]);
        acc[0][1] = mfma16x16x4(b01, y0[k].x, acc[0][1]);
        if (MT == 2) {
            acc[MT - 1][0] = mfma16x16x4(b00, y1[k].x, acc[MT - 1][0]);
            acc[MT - 1][1] = mfma16x16x4(b01, y1[k].x, acc[MT - 1][1]);
        }
        acc2[0][0] = mfma16x16x4(b10, y0[k].y, acc2[0][0]);
        acc2[0][1] = mfma16x16x4(b11, y0[k].y, acc2[0][1]);
        if (MT == 2) {
            acc2[MT - 1][0] = mfma16x16x4(b10, y1[k].y, acc2[MT - 1][0]);
            acc2[MT - 1][1] = mfma16x16x4(b11, y1[k].y, acc2[MT - 1][1]);
        }
    };
#pragma unroll
    for (int k = 0; k < R - 1; ++k)
        if (k < nch) load(k, k);
    pre();
    for (int t = 0; t < nch; t += R) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (t + k + R - 1 < nch) load(t + k + R - 1, (k + R - 1) % R);
            if (t + k < nch) mma(k);
        }
    }
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] += acc2[a][b];
}

template <int KW, int MT = 2>
__device__ __forceinline__ void wpass_tile(const Dims &d, const double *__restrict__ Y,
                                           const double *__restrict__ Lam, const double *__restrict__ omega,
                                           double *__restrict__ W, int w, int kt) {
    const int nrb = d.NP / (64 * MT);                // row blocks per shard
    const int m = w / nrb, rb = w % nrb;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i0 = rb * 64 * MT + wave * 16 * MT;
    const int r = lane & 15, q = lane >> 4;
    d4 acc[MT][2];
    wpass_acc<KW, MT>(d, Y, Lam, omega, m, i0, kt, acc, [] {});
    // acc[a][tb][g] = W[i0 + 16a + r][32 kt + 8g + 2q + tb]: one 16-byte pair per (a, g)
#pragma unroll
    for (int a = 0; a < MT; ++a) {
        double *Wt = W + ((size_t)m * d.NP + i0 + 16 * a + r) * KW + 32 * kt + 2 * q;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            d2 v;
            v.x = acc[a][0][g];
            v.y = acc[a][1][g];
            *reinterpret_cast<d2 *>(Wt + 8 * g) = v;
        }
    }
}

// ============================================================================
// C pass, one wave's share of a block's reduction over rows i (k_cpass: block = (shard m,
// 32-column tile of [Y | eta]) x (32-column tile kt of eta)).
// Lane (r, q) loads 16 B: Y[i][c0+2r .. +1] and eta[i][2r .. +1] (formed on the
// fly from X and Z), i = 4s + q, so the MFMA tiles are even/odd columns x
// even/odd k.  Register double-buffered prefetch, 4 k-steps per batch (a ring of 3: same
// time at c3 and c4, 180 VGPRs).
// ============================================================================
// IS_E: the A operand is eta itself, columns te*32.. (Yp = nullptr; Xa/Za point at
// them); SAME_T: te == kt, so the A operand is the B operand (no extra loads).
// PS: the block computes only the k columns of parity par (acc[.][0]); same per-element order
// ETA (wide, KW > KP): Xp / Xa point at eta itself (formed once per iteration by k_eta into the free W
// buffer, with the same eta_of), Zp / Za unused: one load per operand instead of two
template <int KW, bool IS_E, bool SAME_T, bool PS = false>
__device__ __forceinline__ void cpass_wave(const Dims &d, const double *__restrict__ Yp,
                                           const double *__restrict__ Xp,
                                           const double *__restrict__ Zp,
                                           const double *__restrict__ Xa,
                                           const double *__restrict__ Za, int s0, int nsw,
                                           int q, d4 (&acc)[2][2], int par = 0) {
    constexpr bool EXTRA = IS_E && !SAME_T, ETA = KW > KP;
    d2 yA[4], xA[4], zA[4], yB[4], xB[4], zB[4];
    auto load = [&](int s, d2 (&y)[4], d2 (&x)[4], d2 (&z)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = 4 * (s + u) + q;
            x[u] = *reinterpret_cast<const d2 *>(Xp + (size_t)i * KW);
            if (!ETA) z[u] = *reinterpret_cast<const d2 *>(Zp + (size_t)i * KW);
            if (!IS_E) {
                y[u] = *reinterpret_cast<const d2 *>(Yp + (size_t)i * d.PP);
            } else if (EXTRA) {   // eta of tile te, formed into y
                const d2 xa = *reinterpret_cast<const d2 *>(Xa + (size_t)i * KW);
                if (ETA) {
                    y[u] = xa;
                } else {   // compiled for KW == KP only, where te == kt always (one eta column tile)
                    const d2 za = *reinterpret_cast<const d2 *>(Za + (size_t)i * KW);
                    y[u].x = eta_of(d.sr, d.s1r, xa.x, za.x);
                    y[u].y = eta_of(d.sr, d.s1r, xa.y, za.y);
                }
            }
        }
    };
    auto mma = [&](d2 (&y)[4], d2 (&x)[4], d2 (&z)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double e0 = ETA ? x[u].x : eta_of(d.sr, d.s1r, x[u].x, z[u].x);
            const double e1 = ETA ? x[u].y : eta_of(d.sr, d.s1r, x[u].y, z[u].y);
            const double a0 = (IS_E && SAME_T) ? e0 : y[u].x, a1 = (IS_E && SAME_T) ? e1 : y[u].y;
            if constexpr (PS) {
                const double ep = par ? e1 : e0;
                acc[0][0] = mfma16x16x4(a0, ep, acc[0][0]);
                acc[1][0] = mfma16x16x4(a1, ep, acc[1][0]);
            } else {
                acc[0][0] = mfma16x16x4(a0, e0, acc[0][0]);
                acc[0][1] = mfma16x16x4(a0, e1, acc[0][1]);
                acc[1][0] = mfma16x16x4(a1, e0, acc[1][0]);
                acc[1][1] = mfma16x16x4(a1, e1, acc[1][1]);
            }
        }
    };
    const int nb = nsw >> 2;
    load(s0, yA, xA, zA);
    for (int b = 0; b < nb; b += 2) {
        if (b + 1 < nb) load(s0 + 4 * (b + 1), yB, xB, zB);
        mma(yA, xA, zA);
        if (b + 2 < nb) load(s0 + 4 * (b + 2), yA, xA, zA);
        if (b + 1 < nb) mma(yB, xB, zB);
    }
}

}  // namespace dcfm
