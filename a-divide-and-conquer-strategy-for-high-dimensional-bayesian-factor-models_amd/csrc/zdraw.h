// The narrow (K <= 32) Z draw and per-shard X message as fp64 MFMA chains.   dc:101-107,121-123
//   Z' = M1 W' + M2 X' + U eps'      (the shard's operators ZM, zx_ops.h; columns = rows i)
//   S' = W' + NA Z'                  (S_i = Xmsg'(Y_i - sqrt(1-rho) L Z_i))
// One 16-row tile per wave.  Operand lane map:
// lane (c = lane&15, q = lane>>4) holds W[i0+c][8t+2q .. +1] (k-steps 2t+e); the three
// products of Z' accumulate in separate registers (6 independent MFMA chains per wave,
// 4 waves per SIMD: fp64 MFMA needs many chains in flight) and are added at the end
// ((M1 W' + M2 X') + U eps').  The f64 C/D layout of Z' (row = q + 4r) is directly the B
// operand of the NA Z' product (k-step r), so nothing crosses LDS.
// zdraw_tile (k_zdraw) takes W from HBM; wpass_z_tile (k_wcol) from the W pass's accumulators.
#pragma once
#include "dcfm_internal.h"
#include "linalg.h"
#include "handoff.h"
#include "draws.h"
#include "ypass.h"
#include "wstamp.h"

namespace dcfm {

constexpr int ZDRAW_SMEM = 4 * KP * (KP + 1);
constexpr int ZROWS = 128, ZTHREADS = 512;     // rows and threads per k_zdraw block

// The draw of 16 rows from the operand registers — lane (c, q) holds row i = (its tile's row c):
// wv[t] = W[i][8t+2q .. +1], xv[t] = X[i][..], ev[t] = eps[i][..] (k-steps 2t + e) — and the
// shard's operators Ms = {M1, M2, U, NA} in LDS.  The S' = W' + NA Z' product takes its A rows
// in the order pi(16 mt + c) = 8 (c >> 2) + 2 (c & 3) + mt, so its C/D registers hold exactly the
// features of wv (the accumulators start from W without a reload, and a lane stores S_i[8g+2q ..
// +1] as one 16-byte pair); every element keeps its products and their order, so the values
// are those of the unpermuted product.  Shared by k_zdraw (W from HBM) and k_wcol's
// fused W pass (W' still in the W-pass accumulators), which therefore give the same bits.
__device__ __forceinline__ void zdraw_rows(const Dims &d, const double (*Ms)[KP][KP + 1], const d2 (&wv)[4],
                                           const d2 (&xv)[4], const d2 (&ev)[4], double *__restrict__ Zr,
                                           double *__restrict__ Sr, bool live, int c, int q) {
    d4 zw[2], zx[2], ze[2], as[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) zw[mt] = zx[mt] = ze[mt] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        double mo[2][3][2];   // this chunk's operator values, read before its 12 MFMAs
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int mat = 0; mat < 3; ++mat)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) mo[e][mat][mt] = Ms[mat][16 * mt + c][8 * t + 2 * q + e];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double we = e ? wv[t].y : wv[t].x, xe = e ? xv[t].y : xv[t].x;
            const double ee = e ? ev[t].y : ev[t].x;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                zw[mt] = mfma16x16x4(mo[e][0][mt], we, zw[mt]);
                zx[mt] = mfma16x16x4(mo[e][1][mt], xe, zx[mt]);
                ze[mt] = mfma16x16x4(mo[e][2][mt], ee, ze[mt]);
            }
        }
    }
    d4 az[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        az[mt] = (zw[mt] + zx[mt]) + ze[mt];
#pragma unroll
        for (int g = 0; g < 4; ++g) as[mt][g] = mt ? wv[g].y : wv[g].x;     // W[i][8g + 2q + mt]
    }
    // S' = W' + NA Z' (rows of NA in the order pi)
    const int prow = 8 * (c >> 2) + 2 * (c & 3);
#pragma unroll
    for (int mt2 = 0; mt2 < 2; ++mt2)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int kk = 16 * mt2 + 4 * g + q;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) as[mt] = mfma16x16x4(Ms[3][prow + mt][kk], az[mt2][g], as[mt]);
        }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int k = 16 * mt + q + 4 * g;
            if (live) Zr[k] = (k < d.K) ? az[mt][g] : 0.0;
        }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        d2 v;
        v.x = live ? as[0][g] : 0.0;
        v.y = live ? as[1][g] : 0.0;
        *reinterpret_cast<d2 *>(Sr + 8 * g + 2 * q) = v;
    }
}

// block = (shard m, ZT / 4 rows), ZT / 64 waves.
// ZT threads = ZT / 4 rows per block: 256 (64-row blocks) where 128-row ones would leave CUs
// idle (a few shards per rank); rows are independent, so the choice changes no bit
template <int ZT = ZTHREADS>
__device__ __forceinline__ void zdraw_tile(const Dims &d, const double *__restrict__ W,
                                           const double *__restrict__ ZM, const double *__restrict__ X,
                                           double *__restrict__ Z, double *__restrict__ Sp, const DrawsDev &dr,
                                           int64_t iter, int w, double *smem) {
    double (*Ms)[KP][KP + 1] = reinterpret_cast<double (*)[KP][KP + 1]>(smem);   // M1, M2, U, NA
    const int nrb = d.NP / (ZT / 4);
    const int m = w / nrb, rb = w % nrb;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 15, q = lane >> 4;
    const int mg = d.shard0 + m;
    const int i0 = rb * (ZT / 4) + wave * 16;
    const int i = i0 + c;
    const bool live = i < d.n;
    // this wave's operands first (in flight while the block stages the operators)
    const double *Wi = W + ((size_t)m * d.NP + i) * KP + 2 * q;
    const double *Xi = X + (size_t)i * KP + 2 * q;
    d2 wv[4], xv[4], ev[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        wv[t] = *reinterpret_cast<const d2 *>(Wi + 8 * t);
        xv[t] = *reinterpret_cast<const d2 *>(Xi + 8 * t);
    }
    // the block's share of the shard's operators, in flight during the draws below (stored to
    // LDS after them: a store per load made the compiler wait for each load in turn)
    constexpr int NU = 4 * KP * KP / ZT;
    double zv[NU];
    {
        const double *Zm = ZM + (size_t)m * 4 * KP * KP;
#pragma unroll
        for (int u = 0; u < NU; ++u) zv[u] = Zm[threadIdx.x + ZT * u];
    }
    z_eps(d, dr, iter, mg, i, live, q, ev);
    {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int e = threadIdx.x + ZT * u;
            const int mat = e / (KP * KP), rem = e % (KP * KP);
            Ms[mat][rem / KP][rem % KP] = zv[u];
        }
    }
    __syncthreads();
    zdraw_rows(d, Ms, wv, xv, ev, Z + ((size_t)m * d.NP + i) * KP, Sp + ((size_t)m * d.NP + i) * KP, live, c, q);
}

// k_wcol's W pass with the Z draw of its rows (fused chain, K <= 32; dc:101-107,121-123): the
// wave's W' tile stays in the accumulators (wpass_acc) and feeds zdraw_rows directly — no W
// round trip through HBM and no k_zdraw launch.  The rows' normals are drawn while the first Y
// chunks are in flight; the shard's operators come from its OPS block of the same launch
// (agent-scope stores, counter SYNC_ZM + m, epoch = the launch's ops epoch), staged once per
// block in LDS after the pass.
template <int MT>
__device__ __forceinline__ void wpass_z_tile(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, int w,
                                             unsigned long long zm_epoch, double *smem) {
    double (*Ms)[KP][KP + 1] = reinterpret_cast<double (*)[KP][KP + 1]>(smem);   // M1, M2, U, NA
    const int nrb = d.NP / (64 * MT);
    const int m = w / nrb, rb = w % nrb;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 15, q = lane >> 4;
    const int mg = d.shard0 + m;
    const int i0 = rb * 64 * MT + wave * 16 * MT;
    d4 acc[MT][2];
    wpass_acc<KP, MT>(d, b.Y, b.Lam, b.omega, m, i0, 0, acc, [] {});
    WSTAMP(2);
    // the operators are normally out long before the pass ends; their loads and the rows' X are
    // issued first, the first tile's normals drawn while they are in flight
    wait_count(b.sync + SYNC_ZM + m, zm_epoch);
    WSTAMP(3);
    constexpr int NU = 4 * KP * KP / 256;
    double zv[NU];
    {
        const double *Zm = b.ZM + (size_t)m * 4 * KP * KP;
#pragma unroll
        for (int u = 0; u < NU; ++u) zv[u] = ld_agent(Zm + threadIdx.x + 256 * u);
    }
    // each tile's X rows after its normals (tile 0's during the operators' staging, tile 1's at its
    // own draw): held across the normals and tile 0's draw they spilled (12 VGPRs at waves_per_eu(3))
    d2 xv[MT][4], ev[MT][4];
    auto load_x = [&](int a) {
        const double *Xi = b.X + (size_t)(i0 + 16 * a + c) * KP + 2 * q;
#pragma unroll
        for (int t = 0; t < 4; ++t) xv[a][t] = *reinterpret_cast<const d2 *>(Xi + 8 * t);
    };
    z_eps(d, dr, iter, mg, i0 + c, i0 + c < d.n, q, ev[0]);   // tile 1's after tile 0's draw (registers)
    load_x(0);                                                  // in flight during the operators' staging
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int e = threadIdx.x + 256 * u;
        const int mat = e / (KP * KP), rem = e % (KP * KP);
        Ms[mat][rem / KP][rem % KP] = zv[u];
    }
    __syncthreads();
    WSTAMP(4);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int a = 0; a < MT; ++a) {
        const int i = i0 + 16 * a + c;
        if (a > 0) {
            load_x(a);
            z_eps(d, dr, iter, mg, i, i < d.n, q, ev[a]);
        }
        d2 wv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            wv[g].x = acc[a][0][g];
            wv[g].y = acc[a][1][g];
        }
        zdraw_rows(d, Ms, wv, xv[a], ev[a], b.Z + ((size_t)m * d.NP + i) * KP, b.Sp + ((size_t)m * d.NP + i) * KP,
                   i < d.n, c, q);
        if (a == 0) WSTAMP(5);
        __builtin_amdgcn_sched_barrier(0);   // one tile's draw at a time (registers)
    }
}

}  // namespace dcfm
