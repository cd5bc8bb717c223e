// Hand-written CDNA4 (gfx950) kernels for one Gibbs iteration of the
// divide-and-conquer factor model (reference divideconquer.m:90-196).
// fp64 throughout (the reference is double precision).  This file holds the __global__
// kernels of the sweep, k_wcol's role dispatch and the launchers; the role bodies are in the
// stage headers: zx_ops.h (K x K operators of the Z / X draws), ypass.h (the two Y passes),
// zdraw.h (Z draw), draws.h (variates), delta.h (column sums, delta / tau chain), lambda.h
// (loading rows; its dc:169-171 is resid.h), handoff.h (hand-off between blocks of one launch).  The covariance assembly
// is assemble.hip, the K > 32 kernels kernels_wide.hip.
//
// Kernel map (per iteration, in order)                         reference lines
//   fused chain (K <= 32), one stream:
//   k_wcol     [Z operators A_m -> M1, M2, U, NA (dc:98-107) | column sums of t-1 (dc:156) |
//              shard sum of A, one rank: Xprec = g I + rho sum A, Rx (dc:112-118)] beside
//              the W pass W_m = Y_m (w o Lambda_m) whose tiles draw Z from their registers
//              and write Z and the shard X message (dc:101-107,121-123), and behind it the
//              loading-row variates of t (dc:142,150,170) for k_lambda
//   several ranks: k_xred (local sum of the X messages) + ONE RCCL all-gather of
//              [column sums | A sum | X message]
//   k_xdraw    X rows (dc:119-128) [+ several ranks: block 0 factors Xprec, Rx from the
//              ranks' A sums]
//   k_cpass    C_m = Y_m' eta_m, E_m = eta_m' eta_m  fp64 MFMA, Y pass 2   dc:133,138,141
//              + in extra blocks the delta / tau chain of t-1 (dc:155-165)
//   k_lambda   per loading row: Q, chol, 3 solves, Lambda_j; psi_j;        dc:140-145,150,
//              SS_j via identity, ps_j, omega_j; psi o L^2 per row         dc:156,169-171
//   side-stream layouts (K > 32, DCFM_FLAG_UNFUSED):
//   k_draws (side stream, one iteration ahead), k_prep / k_xchol (side stream), k_wpass,
//   k_zdraw, k_xred [+ all-gather], k_xdraw, [k_eta,] k_cpass, k_lambda, k_colsum
//   [+ all-gather], k_delta
//   (Plam = psi o tau' of dc:175-177 is formed where it is read: in the next
//    k_lambda, from the psi and tau arrays — the same single product)
//
// The residual pass of dc:169-170 needs no third read of Y: with C_j = eta'Y_j
// and E = eta'eta already computed for the loading draw,
//   SS_j = sum_i (Y_ij - eta_i Lambda_j')^2 = yy_j - 2 Lambda_j.C_j + Lambda_j E Lambda_j'.
#include "dcfm_internal.h"
#include "philox.h"
#include "linalg.h"
#include "handoff.h"
#include "wstamp.h"
#include "zx_ops.h"
#include "ypass.h"
#include "draws.h"
#include "zdraw.h"
#include "delta.h"
#include "lambda.h"

#include <algorithm>

namespace dcfm {

// k_prep: A_m and the Z-draw operators ZM_m of shard m (zx_ops.h)             dc:98-107
__global__ __launch_bounds__(256) void k_prep(Dims d, const double *__restrict__ Lam,
                                              const double *__restrict__ omega,
                                              double *__restrict__ A, double *__restrict__ ZM) {
    __shared__ double smem[PREP_SMEM];
    prep_shard(d, Lam, omega, A, ZM, blockIdx.x, smem);
}

// k_wpass: W_m = Y_m (w o Lambda_m), Y pass 1 (ypass.h)
template <int KW>
__global__ __launch_bounds__(256) void k_wpass(Dims d, const double *__restrict__ Y,
                                               const double *__restrict__ Lam,
                                               const double *__restrict__ omega,
                                               double *__restrict__ W) {
    // 1-D grid, the KW/32 column tiles of one 128-row block adjacent (same XCD: Y from L2)
    const int w = xcd_remap(blockIdx.x, gridDim.x);
    wpass_tile<KW>(d, Y, Lam, omega, W, w / (KW / 32), w % (KW / 32));
}

// k_zdraw: Z rows and the shard's X message from W in HBM (zdraw.h)      dc:101-107,121-123
// ZT = 256 holds twice the operator staging registers per thread: 2 waves per SIMD (it runs
// only where the launch leaves SIMDs idle anyway) instead of a 128-VGPR cap that spilled
template <int ZT>
__global__ __launch_bounds__(ZT) __attribute__((amdgpu_waves_per_eu(ZT == ZTHREADS ? 4 : 2))) void k_zdraw(Dims d, const double *__restrict__ W,
                                               const double *__restrict__ ZM,
                                               const double *__restrict__ X,
                                               double *__restrict__ Z, double *__restrict__ Sp,
                                               DrawsDev dr, int64_t iter) {
    __shared__ double smem[ZDRAW_SMEM];
    zdraw_tile<ZT>(d, W, ZM, X, Z, Sp, dr, iter, xcd_remap(blockIdx.x, gridDim.x), smem);
}

// ============================================================================
// k_xred: xin[i][k] = sum_m Sp[m][i][k]  (local shards, canonical tree)  dc:120-124
// ============================================================================
__global__ __launch_bounds__(256) void k_xred(Dims d, const double *__restrict__ Sp,
                                              double *__restrict__ xin) {
    const size_t total = (size_t)d.NP * d.kp;
    const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (e >= total) return;
    xin[e] = tree_sum(Sp + e, d.G, total);
}

// ============================================================================
// k_asum: xa = sum_m A_m over local shards (canonical tree), one thread per element.  dc:113-116
// ============================================================================
__global__ __launch_bounds__(256) void k_asum(Dims d, const double *__restrict__ A,
                                              double *__restrict__ xa) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int kk = d.kp * d.kp;
    if (e >= kk) return;
    xa[e] = tree_sum(A + e, d.G, (size_t)kk);
}

// ============================================================================
// k_xchol: Xprec = g*I + rho*sum A (dc:117) and Rx = cholcov(Xprec) (dc:118), on the
// side stream.  Sums the per-rank sums xa_all (k_asum, all-gathered) in the canonical tree
// and writes the X-draw operators XM = {Tx = sqrt(rho) Ux Ux', Ux = Rx^{-T}} (Tx by MFMA).
// ============================================================================
__global__ __launch_bounds__(256) void k_xchol(Dims d, const double *__restrict__ xa_all,
                                               double *__restrict__ XM) {
    __shared__ double smem[XCHOL_SMEM];
    for (int e = threadIdx.x; e < KP * KP; e += 256) {
        xprec_store(d, smem, e, tree_sum(xa_all + e, d.nranks, (size_t)d.xstride));
    }
    __syncthreads();
    xchol_factor(d, XM, smem);
}

// ============================================================================
// k_xdraw: X' = Tx S' + Ux eps' as fp64 MFMA (operators from k_xchol).  S is the sum of
// nsrc [NP][KP] slices in the canonical tree order (TreeSum): the ranks' gathered sums
// (xall), or — one rank, fused chain — the G shard messages Sp themselves, which makes
// k_xred's launch unnecessary.  16 rows per block, 16 waves: wave (t, s) sums source chunk
// s (a power-of-two run of slices, a canonical subtree; xdraw_chunks) of columns
// 8t .. 8t+7 (lane (c, q): row i0 + c, columns 8t + 2q, +1) — the sum is latency-bound, so
// the block keeps 16 waves of loads in flight; wave 0 adds the chunk sums (the tree over the
// chunks) and runs the MFMAs.                                              dc:119-128
// ============================================================================
// source chunks of the X message sum: nch <= 4 runs of `chunk` slices, chunk a power of two
__device__ __forceinline__ void xdraw_chunks(int nsrc, int &nch, int &chunk) {
    chunk = 1;
    while (nsrc / chunk > 4 && (nsrc / chunk) % 2 == 0) chunk *= 2;
    nch = nsrc / chunk;
    if (nch > 4) { nch = 1; chunk = nsrc; }
}
// Roles (xroles & 1, several ranks): block 0 factors Xprec from the ranks' A sums and publishes
// XM (handoff.h); the row blocks sum their messages first and wait for XM only before the MFMAs.
// Row blocks of XD_ROWS rows (the MFMA's other columns padding), every lane summing one part of a
// source chunk: the shard-message sums are bound by the memory parallelism of the CUs that
// issue them (phase stamps: 9 of 14 us with 63 blocks of 16 rows at c3).
constexpr int XD_ROWS = 4;
// Generated X normals (dc:126): wave t < 4 draws Philox pair 4t + q of row i0 + c — one normal2 per
// wave, between the issue of its message loads and their first use — and hands it to wave 0 through
// LDS (evs).  Drawn by wave 0 alone, the four pairs ran ahead of its loads, ~1,200 VALU instructions
// that the other 15 waves waited out at the barrier.  Same counters, formulas and masking.
#ifndef DCFM_XD_SPREAD
#define DCFM_XD_SPREAD 1
#endif
constexpr bool XD_SPREAD = DCFM_XD_SPREAD;   // 0: the A/B baseline, wave 0 draws the four pairs first
constexpr int XD_LDS = 2 * KP * (KP + 1) + 4 * 4 * 64 * 2 + 4 * 64 * 2;   // Ms | part | evs
constexpr int XD_SMEM = XD_LDS > XCHOL_SMEM ? XD_LDS : XCHOL_SMEM;
__global__ __launch_bounds__(1024) void k_xdraw(Dims d, const double *__restrict__ src, int nsrc, size_t sstride,
                                                double *__restrict__ XM,
                                                double *__restrict__ X, DrawsDev dr, int64_t iter, int xroles,
                                                const double *__restrict__ xa, unsigned long long *xm_ctr,
                                                unsigned long long xm_target) {
    __shared__ double smem[XD_SMEM];
    int blk = blockIdx.x;
    if (xroles & 1) {   // producer of XM
        if (blk == 0) {
            for (int e = threadIdx.x; e < KP * KP; e += 1024)   // several ranks: their sums, canonical tree
                xprec_store(d, smem, e, d.nranks > 1 ? tree_sum(xa + e, d.nranks, (size_t)d.xstride) : xa[e]);
            __syncthreads();
            xchol_factor<true>(d, XM, smem);
            signal_count(xm_ctr);
            return;
        }
        blk -= 1;
    }
    double (*Ms)[KP][KP + 1] = reinterpret_cast<double (*)[KP][KP + 1]>(smem);
    d2 (*part)[4][64] = reinterpret_cast<d2 (*)[4][64]>(smem + 2 * KP * (KP + 1));
    d2 (*evs)[64] = reinterpret_cast<d2 (*)[64]>(smem + 2 * KP * (KP + 1) + 4 * 4 * 64 * 2);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int tw = w & 3, sw = w >> 2;                 // column group, source chunk
    const int i0 = blk * XD_ROWS, i = i0 + c;
    const bool live = c < XD_ROWS && i < d.n;          // lanes c >= XD_ROWS pad the MFMA's 16 columns
    const size_t stride = sstride;
    int nch, chunk;
    xdraw_chunks(nsrc, nch, chunk);     // chunk < 1024 (TreeSum levels below); dcfm_create caps g
    d2 sv[4], ev[4];
    if (w == 0 && d.inject) {   // eps of dc:126 (injected draw buffer), in flight during the sum
        const double *nx = dr.NX + ((size_t)(iter - dr.first_iter) * d.n + (live ? i : 0)) * d.K;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int kk = 8 * t + 2 * q;
            ev[t].x = (live && kk < d.K) ? nx[kk] : 0.0;
            ev[t].y = (live && kk + 1 < d.K) ? nx[kk + 1] : 0.0;
        }
    } else if (w == 0 && !XD_SPREAD) {   // generated here (SITE_X, row i): Philox pair 4t + q
        const Rng rng(d.seed);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int kk = 8 * t + 2 * q;
            double n0 = 0.0, n1 = 0.0;
            if (live && kk < d.K) rng.normal2(SITE_X, 0u, (uint32_t)i, (uint32_t)(4 * t + q), (uint32_t)iter, n0, n1);
            ev[t].x = n0;
            ev[t].y = (kk + 1 < d.K) ? n1 : 0.0;
        }
    }
    // one rank: the operators are already out (k_wcol's last arrival): their loads go out before
    // the sums' (two per thread), the LDS stores after
    double xmv[2] = {0.0, 0.0};
    if (!(xroles & 1)) {
#pragma unroll
        for (int u = 0; u < 2; ++u) xmv[u] = XM[threadIdx.x + 1024 * u];
    }
    // wave t = w < 4 (sw = 0 < nch: it has loads below): its pair of the generated normals, ev[t] of wave 0
    auto draw = [&] {
        if (!XD_SPREAD || d.inject || w >= 4) return;
        const int kk = 8 * w + 2 * q;
        double n0 = 0.0, n1 = 0.0;
        if (live && kk < d.K) Rng(d.seed).normal2(SITE_X, 0u, (uint32_t)i, (uint32_t)(4 * w + q), (uint32_t)iter, n0, n1);
        evs[w][lane] = d2{n0, (kk + 1 < d.K) ? n1 : 0.0};
    };
    if (sw < nch) {
        if (chunk >= 2) {   // lane c sums part c / XD_ROWS (a canonical subtree) of the chunk for row c % XD_ROWS
            // the parts split only a power-of-two chunk (np | chunk, each part a canonical
            // subtree); a chunk of any other size (xdraw_chunks: nch = 1, chunk = nsrc, e.g.
            // g = 5 or 10 shards) is summed whole by the h == 0 lanes
            constexpr int NPART = 16 / XD_ROWS;
            const int np = (chunk & (chunk - 1)) ? 1 : (chunk < NPART ? chunk : NPART), per = chunk / np;
            const int rr = c % XD_ROWS, h = c / XD_ROWS;
            const bool rl = i0 + rr < d.n && h < np;
            const double *p = src + (size_t)(sw * chunk + (h < np ? h : 0) * per) * stride +
                              (size_t)(i0 + rr < d.n ? i0 + rr : i0) * KP + 8 * tw + 2 * q;
            // a lane with no part sums zeros (the trip counts stay wave-uniform); the draw sits behind the
            // first batch's loads
            d2 v = tree_sum_f<d2, 8, 10>(per, [&](int rk) {
                return rl ? *reinterpret_cast<const d2 *>(p + (size_t)rk * stride) : d2{0.0, 0.0};
            }, draw);
            for (int o = 1; o < np; o <<= 1) {   // adjacent parts pairwise: the canonical tree over the parts
                d2 u;
                u.x = __shfl_down(v.x, o * XD_ROWS, 16);
                u.y = __shfl_down(v.y, o * XD_ROWS, 16);
                v.x = v.x + u.x;
                v.y = v.y + u.y;
            }
            part[sw][tw][lane] = h == 0 ? v : d2{0.0, 0.0};
        } else {
            const double *p = src + (size_t)sw * chunk * stride + (size_t)(live ? i : i0) * KP + 8 * tw + 2 * q;
            const d2 v = live ? *reinterpret_cast<const d2 *>(p) : d2{0.0, 0.0};
            draw();
            part[sw][tw][lane] = v;
        }
    }
    if (xroles & 1) {
        wait_count(xm_ctr, xm_target);       // XM of this launch's block 0
#pragma unroll
        for (int u = 0; u < 2; ++u) xmv[u] = ld_agent(XM + threadIdx.x + 1024 * u);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = threadIdx.x + 1024 * u;
        const int mat = e / (KP * KP), rem = e % (KP * KP);
        Ms[mat][rem / KP][rem % KP] = xmv[u];
    }
    __syncthreads();
    if (w > 0) return;
    if (XD_SPREAD && !d.inject) {
#pragma unroll
        for (int t = 0; t < 4; ++t) ev[t] = evs[t][lane];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        TreeSum<d2, 3> ts;
        for (int k = 0; k < nch; ++k) ts.push(part[k][t][lane]);
        sv[t] = ts.total();
    }
    d4 ax[2];
    ax[0] = ax[1] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int kk = 8 * t + 2 * q + e;
            const double se = e ? sv[t].y : sv[t].x, ee = e ? ev[t].y : ev[t].x;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                ax[mt] = mfma16x16x4(Ms[0][16 * mt + c][kk], se, ax[mt]);
                ax[mt] = mfma16x16x4(Ms[1][16 * mt + c][kk], ee, ax[mt]);
            }
        }
    if (!live) return;
    double *Xr = X + (size_t)i * KP;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int k = 16 * mt + q + 4 * g;
            Xr[k] = (k < d.K) ? ax[mt][g] : 0.0;
        }
}

// ============================================================================
// k_cpass: [C_m | E_m] = [Y_m | eta_m]' eta_m    fp64 MFMA, Y pass 2      dc:133,138,141
// block = (shard m, 32-column tile of [Y | eta]) x (32-column tile kt of eta, the
// fastest index of the 1-D grid); its CP_WAVES waves split the reduction over rows i
// (cpass_wave, ypass.h), partial 32x32 tiles summed in LDS in a fixed order (the canonical
// tree).  The wave count fixes the summation order, so it cannot follow the shard count per
// rank (N ranks reproduce one rank's bits); 8 waves measured g = 8 share 18.2 -> 16.8 us but
// c3 45.5 -> 49.8 us: 4 it is.
// ============================================================================
constexpr int CP_WAVES = 4;
// PS (K <= 32, where the launch would leave CUs idle): each block computes one parity of its
// 32 k columns (twice the blocks, the pair adjacent: Y from L2); per-element order unchanged
// ndel > 0 (fused K <= 32 chain): the last ndel blocks run the previous iteration's delta / tau
// chain (delta_shard, one wave per shard, dc:155-165) beside the pass — it needs only the column
// sums k_wcol (and, several ranks, the packed gather) left, and its ~12 us chain of dependent
// steps would otherwise be the long pole of k_xdraw
// waves_per_eu(3): 164 VGPRs and no AGPRs (without it hipcc took 168 + 32 AGPRs, 2 waves per
// SIMD); measured neutral at c3 and c4 (42.4 vs 42.9 us, 132 vs 135 us), kept for the
// occupancy headroom
template <int KW, bool PS = false>
__global__ __launch_bounds__(64 * CP_WAVES) __attribute__((amdgpu_waves_per_eu(3))) void k_cpass(Dims d, const double *__restrict__ Y,
                                                              const double *__restrict__ X,
                                                              const double *__restrict__ Z,
                                                              double *__restrict__ C, double *__restrict__ E,
                                                              DrawsDev dr, const double *__restrict__ sall,
                                                              DeltaArgs da, int ndel) {
    __shared__ double red[CP_WAVES][32][33];
    const int nbc = gridDim.x - ndel;
    if constexpr (KW == KP) {   // launch_cpass: ndel = 0 for the wide widths
        if ((int)blockIdx.x >= nbc) {
            const int m = (blockIdx.x - nbc) * CP_WAVES + (threadIdx.x >> 6);
            if (m < d.g)
                delta_shard<KP>(d, sall, da.delta_in, da.tau_in, da.delta_out, da.tau_out, dr, da.iter, m, threadIdx.x & 63);
            return;
        }
    }
    // 1-D grid, the KW/32 eta column tiles of one [Y | eta] tile adjacent (same XCD,
    // so the Y tile is fetched once and re-read from L2)
    const int nt = (d.PP + KW) >> 5, nkt = KW / 32;
    int w = xcd_remap(blockIdx.x, nbc);
    const int par = PS ? (w & 1) : 0;
    if (PS) w >>= 1;
    const int kt = w % nkt, m = (w / nkt) / nt, tile = (w / nkt) % nt;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c0 = tile * 32;
    const bool isE = c0 >= d.PP;
    const int te = isE ? (c0 - d.PP) >> 5 : 0;
    const int r = lane & 15, q = lane >> 4;
    const double *Yp = Y + (size_t)m * d.NP * d.PP + c0 + 2 * r;
    // wide: X is eta [G][NP][KW] (k_eta, launch_cpass), so the shard's rows
    constexpr bool ETA = KW > KP;
    const double *Xs = ETA ? X + (size_t)m * d.NP * KW : X;
    const double *Xp = Xs + 32 * kt + 2 * r;
    const double *Zp = Z + (size_t)m * d.NP * KW + 32 * kt + 2 * r;
    const double *Xa = Xs + 32 * te + 2 * r;
    const double *Za = Z + (size_t)m * d.NP * KW + 32 * te + 2 * r;
    const int nsw = d.NP / (4 * CP_WAVES);          // k-steps (4 rows each) per wave
    d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
    if (!isE) cpass_wave<KW, false, false, PS>(d, Yp, Xp, Zp, Xa, Za, wave * nsw, nsw, q, acc, par);
    else if (te == kt) cpass_wave<KW, true, true, PS>(d, Yp, Xp, Zp, Xa, Za, wave * nsw, nsw, q, acc, par);
    else cpass_wave<KW, true, false, PS>(d, Yp, Xp, Zp, Xa, Za, wave * nsw, nsw, q, acc, par);
    // D row rho = q + 4g -> column c0 + 2 rho + ta;  D col r -> k = 2r + tb
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int rho = q + 4 * g;
#pragma unroll
        for (int ta = 0; ta < 2; ++ta) {
            if (PS) {
                red[wave][2 * rho + ta][2 * r + par] = acc[ta][0][g];
            } else {
#pragma unroll
                for (int tb = 0; tb < 2; ++tb) red[wave][2 * rho + ta][2 * r + tb] = acc[ta][tb][g];
            }
        }
    }
    __syncthreads();
    static_assert(CP_WAVES == 4, "tsum is the canonical tree over four waves");
    auto tsum = [&](int a, int b) { return (red[0][a][b] + red[1][a][b]) + (red[2][a][b] + red[3][a][b]); };
    if (KW > KP && isE) {   // wide: E_m in the loading-row kernel's tile layout (etile_index), upper tiles
        double *Em = E + (size_t)m * KW * KW;
        for (int e = threadIdx.x; e < 32 * 32; e += 64 * CP_WAVES) {
            const int a = e >> 5, b = e & 31, R = 32 * te + a, Cc = 32 * kt + b;
            if ((R >> 4) <= (Cc >> 4)) Em[etile_index(KW / 16, R, Cc)] = tsum(a, b);
        }
        return;
    }
    double *out = isE ? (E + (size_t)m * KW * KW + (size_t)(32 * te) * KW + 32 * kt)
                      : (C + ((size_t)m * d.PP + c0) * KW + 32 * kt);
    if (PS) {   // this block's parity of the columns
        for (int e = threadIdx.x; e < 32 * 16; e += 64 * CP_WAVES) {
            const int a = e >> 4, b = 2 * (e & 15) + par;
            out[(size_t)a * KW + b] = tsum(a, b);
        }
        return;
    }
    for (int e = threadIdx.x; e < 32 * 32; e += 64 * CP_WAVES) {
        const int a = e >> 5, b = e & 31;
        out[(size_t)a * KW + b] = tsum(a, b);
    }
}

// k_lambda (loading rows, dc:140-145,150,156,169-171): lambda.h

// k_colsum: sloc[m][k] = sum_{j<P} cpart[m][j][k] (colsum_tile, delta.h)           dc:156
template <int KW>
__global__ __launch_bounds__(256) void k_colsum(Dims d, const double *__restrict__ cpart, double *__restrict__ sloc) {
    __shared__ double smem[8 * 32];
    colsum_tile<KW>(d, cpart, sloc, blockIdx.x, blockIdx.y, smem);
}

// k_delta: the delta / tau chain, one block (one wave) per global shard (delta.h)  dc:154-165
__global__ __launch_bounds__(64) void k_delta(Dims d, const double *__restrict__ sall,
                                               const double *__restrict__ delta_in,
                                               const double *__restrict__ tau_in,
                                               double *__restrict__ delta_out,
                                               double *__restrict__ tau_out,
                                               DrawsDev dr,
                                               int64_t iter) {
    delta_shard<KP>(d, sall, delta_in, tau_in, delta_out, tau_out, dr, iter, blockIdx.x, threadIdx.x);
}

// ============================================================================
// Fused single-stream launches (K <= 32).  Cross-stream event hand-offs cost ~6 us each
// on the critical path, and latency-bound work slows ~2x when it shares CUs with the
// MFMA-bound Y passes, so the small per-shard K x K work rides in the launches of the
// Y passes (k_wcol, k_xdraw, k_cpass) as extra roles (dcfm_run names the plan).
// ============================================================================
// k_wcol (K <= 32): the small per-iteration work that feeds the Z / X draws rides
// in the Y pass's launch.  As separate launches these latency-bound pieces (K x K
// factorisations, shard sums, column sums) cost ~25 us per iteration on the critical path;
// inside k_wpass's launch they run beside the pass.  Roles, in block order (a consumer's
// producers always have lower block ids, so they are dispatched first and a spinning
// consumer can never hold back its producer):
//   OPS    [0, G)      prep_shard(m): A_m (published agent-coherent) and the Z operators ZM_m
//                      of THIS iteration (from the incoming Lambda, omega)           dc:98-107
//   COLSUM [.., +G)    column sums of the PREVIOUS iteration's psi o Lambda^2 (dc:156) for
//                      the delta chain, which runs in a later launch (k_cpass's extra blocks)
//   OPS    [.., +nxs)  wait for every A_m; chunk j's tree sum (a canonical subtree) -> xpart;
//                      the last arrival sums the chunks (canonical tree) into xa (dc:117);
//                      (several ranks: k_xdraw's block 0 factors Xprec from the ranks' sums) dc:112-118
//   WPASS  [.., +nw)   W_m = Y_m (w o Lambda_m) tiles, each drawing Z for its rows and writing
//                      the shard's X message (wpass_z_tile)       dc:101-107,121-123
//   LAMGEN [.., +nlg)  the generated chain's loading-row variates of this iteration for the
//                      k_lambda that follows (lam_draws; VALU work in the slots and issue
//                      cycles the streaming W tiles leave free)      dc:142,150,170
// The hand-offs between the roles: handoff.h.
// ============================================================================
// ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)): the canonical tree of 8 (TreeSum), and of
// any power-of-two n <= 8 when v[n..8) are zero (x + 0 = x)
__device__ __forceinline__ double tree8(const double (&v)[8]) {
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

__device__ __forceinline__ void wcol_body(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, int ops, int colsum,
                                          int wpass, unsigned long long ops_epoch, int xchol, const LamGen &lg,
                                          double *smem) {
    const int G = d.G, nxs = xsum_blocks(G), chunk = G / nxs;
    unsigned long long *chunk_ctr = b.sync + 2;   // per chunk of shards: A_m published
    int blk = blockIdx.x;
    if (ops) {
        if (blk < G) {
            prep_gram<true>(d, b.Lam, b.omega, b.A, b.ZM, blk, smem);
            WSTAMP(2);
            signal_count(chunk_ctr + blk / chunk);   // A_m is out; the operators follow
            prep_ops<true>(d, b.ZM, blk, smem);
            signal_count(b.sync + SYNC_ZM + blk);    // the Z operators are out (the W tiles draw Z)
            return;
        }
        blk -= G;
    }
    if (colsum) {
        if (blk < G) {
            colsum_tile<KP>(d, b.cpart, b.sloc, blk, 0, smem);
            return;
        }
        blk -= G;
    }
    if (ops) {
        if (blk < nxs) {   // chunk j of the shard sum of A, then (last arrival) Xprec and its factors
            const int t = threadIdx.x, j = blk, m0 = j * chunk;   // chunk: a canonical subtree
            constexpr int NU = KP * KP / 256;
            wait_count(chunk_ctr + j, ops_epoch * (unsigned long long)chunk);
            double vs[NU];
            if (chunk <= 8) {                                      // one round: the whole chunk
                double v[NU][8];
#pragma unroll
                for (int u = 0; u < NU; ++u)
#pragma unroll
                    for (int U = 0; U < 8; ++U)
                        v[u][U] = (U < chunk) ? ld_agent(b.A + (size_t)(m0 + U) * KP * KP + t + 256 * u) : 0.0;
#pragma unroll
                for (int u = 0; u < NU; ++u) vs[u] = tree8(v[u]);   // chunk a power of two, or G <= 8
            } else {                                               // groups of 8 (subtrees), then their tree
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    TreeSum<double, 6> ts;
                    for (int k = 0; k < chunk; k += 8) {
                        double v[8];
#pragma unroll
                        for (int U = 0; U < 8; ++U) v[U] = ld_agent(b.A + (size_t)(m0 + k + U) * KP * KP + t + 256 * u);
                        ts.push(tree8(v));
                    }
                    vs[u] = ts.total();
                }
            }
            if (nxs > 1) {   // several chunks: publish, the last arrival goes on
#pragma unroll
                for (int u = 0; u < NU; ++u) st_agent(b.xpart + (size_t)j * KP * KP + t + 256 * u, vs[u]);
                if (!last_arrival(b.ticket, (unsigned)nxs, reinterpret_cast<unsigned *>(smem))) return;
            }
            double xs[NU];
            if (nxs <= 8) {   // canonical tree over the chunk sums: every load in flight at once
                              // (a round trip per u cost ~1.3 us each); tree8 with zeros past nxs
                              // is TreeSum's order for any nxs <= 8
                double v[NU][8];
#pragma unroll
                for (int u = 0; u < NU; ++u)
#pragma unroll
                    for (int U = 0; U < 8; ++U)
                        v[u][U] = (U < nxs) ? (U == j ? vs[u] : ld_agent(b.xpart + (size_t)U * KP * KP + t + 256 * u))
                                            : 0.0;
#pragma unroll
                for (int u = 0; u < NU; ++u) xs[u] = tree8(v[u]);
            } else {   // a non-power-of-two G: the chunks are single shards and nxs = G exceeds
                       // 8: groups of 8 into a TreeSum
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    TreeSum<double, 8> ts;
                    for (int k = 0; k < nxs; k += 8) {
                        double v[8];
#pragma unroll
                        for (int U = 0; U < 8; ++U)
                            v[U] = (k + U < nxs) ? (k + U == j ? vs[u] : ld_agent(b.xpart + (size_t)(k + U) * KP * KP + t + 256 * u))
                                                 : 0.0;
                        static_for<8>([&](auto U) { if (k + U < nxs) ts.push(v[U]); });
                    }
                    xs[u] = ts.total();
                }
            }
            if (!xchol) {   // several ranks: the local sum into the packed message (all-gathered next)
#pragma unroll
                for (int u = 0; u < NU; ++u) b.xa[t + 256 * u] = xs[u];
                return;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < NU; ++u) xprec_store(d, smem, t + 256 * u, xs[u]);
            __syncthreads();
            xchol_factor(d, b.XM, smem);              // Xprec = g I + rho sum A (dc:117), Rx (dc:118)
            return;
        }
        blk -= nxs;
    }
    if (wpass) {   // 1: 128-row blocks, 2: 64-row blocks (wcol_wpass_mode); W' -> the Z draw
        const int nw = (d.NP / (64 * (3 - wpass))) * d.G;
        if (blk < nw) {
            if (wpass == 2) wpass_z_tile<1>(d, b, dr, iter, xcd_remap(blk, nw), ops_epoch, smem);
            else wpass_z_tile<2>(d, b, dr, iter, xcd_remap(blk, nw), ops_epoch, smem);
            return;
        }
        blk -= nw;
    }
    // the loading-row variates of this iteration (generated chain), behind every other role
    if (blk < lg.b_total) lam_draws(d, lg, iter, blk * LAM_GEN_THREADS + (int)threadIdx.x, lg.b_total * LAM_GEN_THREADS);
}

#ifndef DCFM_WCOL_WPE
#define DCFM_WCOL_WPE 3
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DCFM_WCOL_WPE))) void k_wcol(Dims d, Bufs b, DrawsDev dr, int64_t iter, int ops, int colsum,
                                              int wpass, unsigned long long ops_epoch, int xchol, LamGen lg) {
    __shared__ double smem[PREP_SMEM];
#ifdef DCFM_WSTAMPS
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_readcyclecounter();
#endif
    wcol_body(d, b, dr, iter, ops, colsum, wpass, ops_epoch, xchol, lg, smem);
#ifdef DCFM_WSTAMPS
    if (wpass && threadIdx.x == 0 && blockIdx.x < 8192) {
        g_wstamps[blockIdx.x][0] = t0;
        g_wstamps[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
        g_wstamps[blockIdx.x][6] = c0;                                 // shader clock: the block's mean frequency
        g_wstamps[blockIdx.x][7] = __builtin_readcyclecounter();
    }
#endif
}

// eta = sqrt(rho) X + sqrt(1-rho) Z, formed once per iteration for the wide k_cpass    dc:133
__global__ __launch_bounds__(256) void k_eta(Dims d, const double *__restrict__ X,
                                             const double *__restrict__ Z, double *__restrict__ eta) {
    const size_t total = (size_t)d.G * d.NP * d.kp;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total;
         e += (size_t)gridDim.x * blockDim.x) {
        const size_t ik = e % ((size_t)d.NP * d.kp);
        eta[e] = eta_of(d.sr, d.s1r, X[ik], Z[e]);
    }
}

// k_draws: one iteration's variates into the draw buffers (draws.h)
template <bool GAMMAS>
__global__ __launch_bounds__(256) void k_draws(Dims d, DrawsDev dr, int64_t iter) {
    const DrawPlan pl = draw_plan(d);
    draws_block<GAMMAS>(d, dr, iter, pl, blockIdx.x + (GAMMAS ? 0 : pl.b_gpsi));
}

// variate e at counter (site, shard, row = e / width, index = e % width, iter)
__global__ __launch_bounds__(256) void k_rng_fill(uint64_t seed, int kind, double shape, int site,
                                                  int shard, int64_t iter, int64_t count, int width,
                                                  double *__restrict__ out) {
    const Rng rng(seed);
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count;
         e += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(e / width), k = (uint32_t)(e % width);
        out[e] = kind == 0 ? rng.normal(site, shard, row, k, (uint32_t)iter)
                           : rng.gamma(shape, site, shard, row, k, (uint32_t)iter);
    }
}

// ============================================================================
// launchers
// ============================================================================
// kp == 32: the register-blocked narrow kernels of this file; kp = 64 / 128: the
// wide kernels of kernels_wide.hip (wide::).  Layout-generic kernels are templated.
void launch_prep(const Dims &d, const Bufs &b, hipStream_t s) {
    if (d.kp != KP) return wide::launch_prep(d, b, s);
    hipLaunchKernelGGL(k_prep, dim3(d.G), dim3(256), 0, s, d, b.Lam, b.omega, b.A, b.ZM);
}
void launch_wpass(const Dims &d, const Bufs &b, hipStream_t s) {
    const dim3 grid((d.NP / 128) * d.G * (d.kp / 32));
    switch (d.kp) {
    case 32: hipLaunchKernelGGL(k_wpass<32>, grid, dim3(256), 0, s, d, b.Y, b.Lam, b.omega, b.W); break;
    case 64: hipLaunchKernelGGL(k_wpass<64>, grid, dim3(256), 0, s, d, b.Y, b.Lam, b.omega, b.W); break;
    default: hipLaunchKernelGGL(k_wpass<128>, grid, dim3(256), 0, s, d, b.Y, b.Lam, b.omega, b.W); break;
    }
}
void launch_zdraw(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, hipStream_t s) {
    if (d.kp != KP) return wide::launch_zdraw(d, b, dr, iter, s);
    if ((d.NP / ZROWS) * d.G < 256)   // 64-row blocks (zdraw_tile)
        hipLaunchKernelGGL(k_zdraw<256>, dim3((d.NP / 64) * d.G), dim3(256), 0, s, d, b.W, b.ZM, b.X, b.Z, b.Sp, dr, iter);
    else
        hipLaunchKernelGGL(k_zdraw<ZTHREADS>, dim3((d.NP / ZROWS) * d.G), dim3(ZTHREADS), 0, s, d, b.W, b.ZM, b.X, b.Z,
                           b.Sp, dr, iter);
}
// k_wcol launch (K <= 32)
void launch_wcol(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, bool ops, bool colsum, bool wpass,
                 unsigned long long ops_epoch, hipStream_t s, bool lamgen) {
    static_assert(LAM_GEN_THREADS == 256, "k_wcol blocks are 256 threads");
    LamGen lg = {};
    if (lamgen && b.ldraw) lg = lam_gen_plan(d, b.ldraw);
    // W pass tiles: 64-row blocks up to one 128-row block per CU (the g = 32 share of c3: 256
    // blocks; 64-row ones measured 2.8 % faster there, 128-row ones faster at c3's 512)
    const int wmode = (d.NP / 128) * d.G <= 256 ? 2 : 1;
    const int nb = (ops ? d.G + xsum_blocks(d.G) : 0) + (colsum ? d.G : 0) + (wpass ? (d.NP / (64 * (3 - wmode))) * d.G : 0);
    if (nb + lg.b_total == 0) return;
    hipLaunchKernelGGL(k_wcol, dim3(nb + lg.b_total), dim3(256), 0, s, d, b, dr, iter, ops ? 1 : 0, colsum ? 1 : 0,
                       wpass ? wmode : 0, ops_epoch, d.coll ? 0 : 1, lg);
}
void launch_xred(const Dims &d, const Bufs &b, hipStream_t s) {
    const int total = d.NP * d.kp;
    hipLaunchKernelGGL(k_xred, dim3(cdiv(total, 256)), dim3(256), 0, s, d, b.Sp, b.xin);
}
void launch_asum(const Dims &d, const Bufs &b, hipStream_t s) {
    hipLaunchKernelGGL(k_asum, dim3(cdiv(d.kp * d.kp, 256)), dim3(256), 0, s, d, b.A, b.xa);
}
void launch_xchol(const Dims &d, const Bufs &b, hipStream_t s) {
    if (d.kp != KP) return wide::launch_xchol(d, b, s);
    hipLaunchKernelGGL(k_xchol, dim3(1), dim3(256), 0, s, d, d.coll ? b.xa_all : b.xa, b.XM);
}
void launch_xdraw(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, hipStream_t s,
                  bool from_shards) {
    if (d.kp != KP) return wide::launch_xdraw(d, b, dr, iter, s);
    const dim3 grid(cdiv(d.n, XD_ROWS));
    const size_t st = (size_t)d.NP * KP;
    if (from_shards)   // one rank: sum the G shard messages here (no k_xred)
        hipLaunchKernelGGL(k_xdraw, grid, dim3(1024), 0, s, d, b.Sp, d.G, st, b.XM, b.X, dr, iter, 0, nullptr, nullptr,
                           0ull);
    else
        hipLaunchKernelGGL(k_xdraw, grid, dim3(1024), 0, s, d, b.xall, d.nranks, st, b.XM, b.X, dr, iter, 0, nullptr,
                           nullptr, 0ull);
}
void launch_xdraw_mr(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, unsigned long long xm_epoch,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_xdraw, dim3(1 + cdiv(d.n, XD_ROWS)), dim3(1024), 0, s, d, b.xall, d.nranks, (size_t)d.xstride,
                       b.XM, b.X, dr, iter, 1, b.xa_all, b.sync, xm_epoch);
}
void launch_cpass(const Dims &d, const Bufs &b, hipStream_t s, const DrawsDev &dr, const double *delta_in,
                  const double *tau_in, double *delta_out, double *tau_out, int64_t delta_iter) {
    const dim3 grid(((d.PP + d.kp) / 32) * d.G * (d.kp / 32));
    DeltaArgs da;
    da.delta_in = delta_in; da.tau_in = tau_in; da.delta_out = delta_out; da.tau_out = tau_out;
    da.iter = delta_iter;
    const int ndel = (delta_in && d.kp == KP) ? cdiv(d.g, CP_WAVES) : 0;
    switch (d.kp) {
    case 32:
        // a few shards per rank: split the k columns by parity (k_cpass PS) below 128 blocks
        // (c3's g = 8 share, 88 blocks: +7 %; the g = 16 / 32 shares, 176 / 352: -4 / -2 %)
        if (grid.x < 128)
            hipLaunchKernelGGL((k_cpass<32, true>), dim3(2 * grid.x + ndel), dim3(64 * CP_WAVES), 0, s, d, b.Y,
                               b.X, b.Z, b.C, b.E, dr, b.sall, da, ndel);
        else
            hipLaunchKernelGGL((k_cpass<32, false>), dim3(grid.x + ndel), dim3(64 * CP_WAVES), 0, s, d, b.Y, b.X,
                               b.Z, b.C, b.E, dr, b.sall, da, ndel);
        break;
    // wide: eta formed once (k_eta into W, free after k_zdraw) instead of in each of the shard's column
    // tiles from X and Z: their two 2 MB panels shared the XCD's L2 with the Y stream (c4: 358 MB)
    case 64:
        launch_eta(d, b, b.W, s);
        hipLaunchKernelGGL(k_cpass<64>, grid, dim3(256), 0, s, d, b.Y, b.W, b.Z, b.C, b.E, dr, b.sall, da, 0);
        break;
    default:
        launch_eta(d, b, b.W, s);
        hipLaunchKernelGGL(k_cpass<128>, grid, dim3(256), 0, s, d, b.Y, b.W, b.Z, b.C, b.E, dr, b.sall, da, 0);
        break;
    }
}
void launch_lambda(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter,
                   const double *tau_cur, const double *plam_src, hipStream_t s, bool gen, double kappa_max,
                   const SaveArgs &sv) {
    if (d.kp != KP) return wide::launch_lambda(d, b, dr, iter, tau_cur, plam_src, s, kappa_max);   // k_save saves
    const LamDraws ld = lam_draws_at(d, b, dr, iter, gen);
    const dim3 grid(cdiv(d.P, LAM_ROWS), d.G);
#define LAUNCH_LAM(KE)                                                                                       \
    hipLaunchKernelGGL(k_lambda<KE>, grid, dim3(64), 0, s, d, b.C, b.E, b.yy, tau_cur, b.Lam, b.psi, plam_src, \
                       b.ps, b.omega, b.cpart, ld, b.Y, b.X, b.Z, kappa_max, sv)
    // the factor width rounded up to an instantiated one (rows >= K are identity padding)
    if (d.K <= 8) LAUNCH_LAM(8);
    else if (d.K <= 16) LAUNCH_LAM(16);
    else if (d.K <= 20) LAUNCH_LAM(20);
    else if (d.K <= 24) LAUNCH_LAM(24);
    else if (d.K <= 30) LAUNCH_LAM(30);
    else LAUNCH_LAM(32);
#undef LAUNCH_LAM
}
void launch_colsum(const Dims &d, const Bufs &b, hipStream_t s) {
    const dim3 grid(d.G, d.kp / 32);
    switch (d.kp) {
    case 32: hipLaunchKernelGGL(k_colsum<32>, grid, dim3(256), 0, s, d, b.cpart, b.sloc); break;
    case 64: hipLaunchKernelGGL(k_colsum<64>, grid, dim3(256), 0, s, d, b.cpart, b.sloc); break;
    default: hipLaunchKernelGGL(k_colsum<128>, grid, dim3(256), 0, s, d, b.cpart, b.sloc); break;
    }
}
void launch_delta(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter,
                  const double *delta_in, const double *tau_in, double *delta_out, double *tau_out,
                  hipStream_t s) {
    if (d.kp != KP) return wide::launch_delta(d, b, dr, iter, delta_in, tau_in, delta_out, tau_out, s);
    hipLaunchKernelGGL(k_delta, dim3(d.g), dim3(64), 0, s, d, b.sall, delta_in, tau_in, delta_out,
                       tau_out, dr, iter);
}
void launch_eta(const Dims &d, const Bufs &b, double *eta_out, hipStream_t s) {
    const size_t total = (size_t)d.G * d.NP * d.kp;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(k_eta, dim3(grid), dim3(256), 0, s, d, b.X, b.Z, eta_out);
}
void launch_draws(const Dims &d, const DrawsDev &dr, int64_t iter, hipStream_t s) {
    const DrawPlan pl = draw_plan(d);
    hipLaunchKernelGGL(k_draws<true>, dim3(pl.b_gpsi), dim3(256), 0, s, d, dr, iter);
    hipLaunchKernelGGL(k_draws<false>, dim3(pl.total - pl.b_gpsi), dim3(256), 0, s, d, dr, iter);
}
void launch_rng_fill(uint64_t seed, int kind, double shape, int site, int shard, int64_t iter,
                     int64_t count, int width, double *out, hipStream_t s) {
    const int grid = (int)std::min<int64_t>((count + 255) / 256, 8192);
    hipLaunchKernelGGL(k_rng_fill, dim3(grid > 0 ? grid : 1), dim3(256), 0, s, seed, kind, shape, site,
                       shard, iter, count, width, out);
}

// NaN / Inf sentinel (DCFM_ERR_NUMERIC): after a dcfm_run, every non-finite value of the
// state a later iteration reads (Lambda, ps, omega, X, tau) sets *flag (sticky until the
// next set_state / init_state).  A NaN anywhere in a sweep reaches these within one
// iteration (SS_j -> ps_j -> omega_j; X -> eta -> Lambda).  One pass over ~6 MB at c3.
__device__ __forceinline__ bool bad(double v) { return !(fabs(v) <= 1.7976931348623157e308); }
__global__ __launch_bounds__(256) void k_finite(Dims d, const double *__restrict__ Lam,
                                                const double *__restrict__ ps, const double *__restrict__ omega,
                                                const double *__restrict__ X, const double *__restrict__ tau,
                                                int *__restrict__ flag) {
    const size_t nL = (size_t)d.G * d.PP * d.kp, nP = (size_t)d.G * d.PP, nX = (size_t)d.NP * d.kp,
                 nT = (size_t)d.g * d.kp;
    bool any = false;
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < nL; e += (size_t)gridDim.x * 256) any |= bad(Lam[e]);
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < nP; e += (size_t)gridDim.x * 256)
        any |= bad(ps[e]) || bad(omega[e]);
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < nX; e += (size_t)gridDim.x * 256) any |= bad(X[e]);
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < nT; e += (size_t)gridDim.x * 256) any |= bad(tau[e]);
    if (any) *flag = 1;   // benign race: every writer stores 1
}
void launch_finite(const Dims &d, const Bufs &b, const double *tau_cur, int *flag, hipStream_t s) {
    hipLaunchKernelGGL(k_finite, dim3(128), dim3(256), 0, s, d, b.Lam, b.ps, b.omega, b.X, tau_cur, flag);
}

// dst[i] = sum_k src[k * count + i] in slice order (the loopback all-reduce)
__global__ __launch_bounds__(256) void k_sum_slices(const double *__restrict__ src, int ns, size_t count,
                                                   double *__restrict__ dst) {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        double v = 0.0;
        for (int k = 0; k < ns; ++k) v += src[(size_t)k * count + i];
        dst[i] = v;
    }
}
void launch_sum_slices(const double *src, int ns, size_t count, double *dst, hipStream_t s) {
    const int grid = (int)std::min<size_t>((count + 255) / 256, 8192);
    hipLaunchKernelGGL(k_sum_slices, dim3(grid > 0 ? grid : 1), dim3(256), 0, s, src, ns, count, dst);
}

}  // namespace dcfm
