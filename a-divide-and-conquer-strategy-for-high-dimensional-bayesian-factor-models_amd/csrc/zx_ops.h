// The narrow (K <= 32) K x K operator work of the Z and X draws: one block per matrix.
//
// Z operators of shard m (k_prep, k_wcol's OPS blocks)                          dc:98-107
//   A_m = (w o Lambda_m)' Lambda_m
//   L = chol(Zprec) lower, Zprec = eye(K) + (1-rho) A_m (cholcov's R = L')
//   U = L^{-1} = R^{-T},  T = U U' = R^{-T} R^{-1}   (quirk Q2: the reference's mean
//   R'\(R\bz) is T bz, its noise R'\z is U z), so with bz = sqrt(1-rho)(W - sqrt(rho) A x):
//     Z = M1 W + M2 x + U eps,   M1 = sqrt(1-rho) T,  M2 = -sqrt(1-rho) sqrt(rho) T A
//     S = W + NA Z,              NA = -sqrt(1-rho) A
// ZM[m] = {M1, M2, U, NA}.  4 waves split the j reduction of A (fp64 MFMA 2x2 tiles).
//
// X operators (k_xchol, k_wcol's last A-sum block, k_xdraw's block 0)           dc:117-118
//   Xprec = g*I + rho*sum A, Rx = cholcov(Xprec);  XM = {Tx = sqrt(rho) Ux Ux', Ux = Rx^{-T}}
#pragma once
#include "dcfm_internal.h"
#include "linalg.h"
#include "handoff.h"
#include "wstamp.h"

namespace dcfm {

constexpr int PREP_SMEM = 4 * KP * (KP + 1) + 3 * TS16;
// prep_gram: A_m (to HBM and LDS part[0]), NA, and Zprec's upper triangle into the
// lower triangle of part[2]; prep_ops: the Z-draw operators from the LDS image.
// PUB: A_m, NA and (prep_ops) the Z operators are published with agent-scope stores (read by other
// blocks of the same launch, k_wcol)
template <bool PUB = false>
__device__ __forceinline__ void prep_gram(const Dims &d, const double *__restrict__ Lam,
                                          const double *__restrict__ omega, double *__restrict__ A,
                                          double *__restrict__ ZM, int m, double *smem) {
    // partial A per wave; later A, U, Zprec/T, scratch
    double (*part)[KP][KP + 1] = reinterpret_cast<double (*)[KP][KP + 1]>(smem);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int r = lane & 15, q = lane >> 4;
    const double *L = Lam + (size_t)m * d.PP * KP;
    const double *w = omega + (size_t)m * d.PP;
    d4 a00 = {0, 0, 0, 0}, a01 = a00, a10 = a00, a11 = a00;
    // rows j, j+1 of chunk tt: (w_j Lambda_ja) is the A operand [Zmsg, dc:98], Lambda_jb the B operand
    auto ld = [&](int tt, d2 &wj, double (&l)[4]) {
        const int j = 8 * tt + 2 * q;
        wj = *reinterpret_cast<const d2 *>(w + j);
        l[0] = L[j * KP + r]; l[1] = L[j * KP + 16 + r];
        l[2] = L[(j + 1) * KP + r]; l[3] = L[(j + 1) * KP + 16 + r];
    };
    auto mm = [&](const d2 &wj, const double (&l)[4]) {
        const double wl0 = l[0] * wj.x, wh0 = l[1] * wj.x, wl1 = l[2] * wj.y, wh1 = l[3] * wj.y;
        a00 = mfma16x16x4(wl0, l[0], a00); a01 = mfma16x16x4(wl0, l[1], a01);
        a10 = mfma16x16x4(wh0, l[0], a10); a11 = mfma16x16x4(wh0, l[1], a11);
        a00 = mfma16x16x4(wl1, l[2], a00); a01 = mfma16x16x4(wl1, l[3], a01);
        a10 = mfma16x16x4(wh1, l[2], a10); a11 = mfma16x16x4(wh1, l[3], a11);
    };
    const int nt = d.PP >> 3;
    int tt = wave;
    for (; tt + 12 < nt; tt += 16) {       // 4 chunks' loads in flight (latency-bound otherwise;
                                           // one round of 10 measured slower: c3 -1.5%)
        d2 wj[4];
        double l[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) ld(tt + 4 * u, wj[u], l[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) mm(wj[u], l[u]);
    }
    for (; tt < nt; tt += 4) {
        d2 wj;
        double l[4];
        ld(tt, wj, l);
        mm(wj, l);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int a = q + 4 * g;
        part[wave][a][r] = a00[g];
        part[wave][a][16 + r] = a01[g];
        part[wave][16 + a][r] = a10[g];
        part[wave][16 + a][16 + r] = a11[g];
    }
    __syncthreads();
    double *Am = A + (size_t)m * KP * KP;
    double *Zm = ZM + (size_t)m * 4 * KP * KP;
    double av[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = t + 256 * u, a = e / KP, b = e % KP;
        av[u] = (part[0][a][b] + part[1][a][b]) + (part[2][a][b] + part[3][a][b]);
        if (PUB) st_agent(Am + e, av[u]);
        else Am[e] = av[u];
        if (PUB) st_agent(Zm + 3 * KP * KP + e, -d.s1r * av[u]);   // NA
        else Zm[3 * KP * KP + e] = -d.s1r * av[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = t + 256 * u;
        const int a = e / KP, b = e % KP;
        part[0][a][b] = av[u];                                      // A
        // cholcov reads the upper triangle: lower of Sm = (Zprec upper)'
        if (a <= b) part[2][b][a] = (a == b ? 1.0 : 0.0) + (1.0 - d.rho) * av[u];
    }
    __syncthreads();
}

template <bool PUB = false>
__device__ __forceinline__ void prep_ops(const Dims &d, double *__restrict__ ZM, int m, double *smem) {
    double (*part)[KP][KP + 1] = reinterpret_cast<double (*)[KP][KP + 1]>(smem);
    double *lds_l = smem + 4 * KP * (KP + 1), *lds_u = lds_l + 2 * TS16;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double *Zm = ZM + (size_t)m * 4 * KP * KP;
    if (wave == 0) {                                                // U = L^{-1} -> part[1]
        chol_inv32(part[2], part[1], part[3], lds_l, lds_u, lane);
    }
    __syncthreads();
    if (PUB) WSTAMP(3);
    {   // T = U U' (fp64 MFMA, one 16x16 tile per wave) -> part[2]; M1 = s1r T; U
        const int ti = wave >> 1, tj = wave & 1, j = lane & 15, q = lane >> 4;
        const d4 T = mfma_tile32<true>(part[1], part[1], ti, tj, lane);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int a = 16 * ti + q + 4 * g, c = 16 * tj + j;
            part[2][a][c] = T[g];
            if (PUB) {
                st_agent(Zm + a * KP + c, d.s1r * T[g]);
                st_agent(Zm + 2 * KP * KP + a * KP + c, part[1][a][c]);
            } else {
                Zm[a * KP + c] = d.s1r * T[g];                      // M1
                Zm[2 * KP * KP + a * KP + c] = part[1][a][c];       // U
            }
        }
    }
    __syncthreads();
    {   // M2 = -s1r sr T A (fp64 MFMA)
        const int ti = wave >> 1, tj = wave & 1, j = lane & 15, q = lane >> 4;
        const d4 M = mfma_tile32<false>(part[2], part[0], ti, tj, lane);
        const double s2 = -d.s1r * d.sr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            double *o = Zm + KP * KP + (16 * ti + q + 4 * g) * KP + 16 * tj + j;
            if (PUB) st_agent(o, s2 * M[g]);
            else *o = s2 * M[g];
        }
    }
}

__device__ __forceinline__ void prep_shard(const Dims &d, const double *__restrict__ Lam,
                                           const double *__restrict__ omega, double *__restrict__ A,
                                           double *__restrict__ ZM, int m, double *smem) {
    prep_gram(d, Lam, omega, A, ZM, m, smem);
    prep_ops(d, ZM, m, smem);
}

constexpr int XCHOL_SMEM = 2 * KP * (KP + 1) + TS16 * (KP + 1) + 3 * TS16 + 2;
// smem = {Sm, Us, Wk, lds_l, lds_u, flag}; Sm (lower) holds Xprec's upper triangle on entry
// PUB: XM is published with agent-scope stores (read by other blocks of the same launch, k_xdraw)
template <bool PUB = false>
__device__ __forceinline__ void xchol_factor(const Dims &d, double *__restrict__ XM, double *smem) {
    double (*Sm)[KP + 1] = reinterpret_cast<double (*)[KP + 1]>(smem);
    double (*Us)[KP + 1] = Sm + KP;
    double (*Wk)[KP + 1] = Us + KP;
    double *lds_l = smem + 2 * KP * (KP + 1) + TS16 * (KP + 1), *lds_u = lds_l + 2 * TS16;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (wave == 0) {                       // Ux = Lx^{-1} = Rx^{-T}
        chol_inv32(Sm, Us, Wk, lds_l, lds_u, lane);
    }
    __syncthreads();
    if (wave >= 4) return;                 // blocks of more than 4 waves: the 4 tiles below
    // X = Rx^{-T}(Rx^{-1} sqrt(rho) S + eps) = Tx S + Ux eps,  Tx = sqrt(rho) Ux Ux'
    const int ti = wave >> 1, tj = wave & 1, j = lane & 15, q = lane >> 4;
    const d4 T = mfma_tile32<true>(Us, Us, ti, tj, lane);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int a = 16 * ti + q + 4 * g, c = 16 * tj + j;
        if (PUB) {
            st_agent(XM + a * KP + c, d.sr * T[g]);
            st_agent(XM + KP * KP + a * KP + c, Us[a][c]);
        } else {
            XM[a * KP + c] = d.sr * T[g];
            XM[KP * KP + a * KP + c] = Us[a][c];
        }
    }
}

// Xprec's upper triangle, transposed into the lower triangle of Sm: g I + rho sum A   dc:117
__device__ __forceinline__ void xprec_store(const Dims &d, double *smem, int e, double v) {
    double (*Sm)[KP + 1] = reinterpret_cast<double (*)[KP + 1]>(smem);
    const int a = e / KP, b = e % KP;
    if (a <= b) Sm[b][a] = (a == b ? (double)d.g : 0.0) + d.rho * v;
}

}  // namespace dcfm
