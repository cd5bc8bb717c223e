// Posterior mean of the precision matrix (DCFM_FLAG_PRECISION_MEAN): next to Sigmaout,
//   Prec[a][b] += (1/effsamp) sum_s Sigma(s)^{-1}_ab
// over the saved samples s of a batch, on the assembly stream behind k_assemble.
//
// Per sample Sigma(s) = D + rho Lbar Lbar', D = blockdiag(D_m), D_m = (1 - rho) L_m L_m' + Omega_m (dc:182-192),
// is block-diagonal plus rank K, and so is its inverse.  In the notation of precision.hip, a = 1 - rho,
//   G_m = L_m' Omega_m^{-1} L_m,  B_m = I + a G_m (SPD),  H_m = B_m^{-1} G_m,  S = I + rho sum_m H_m (SPD),
//   M_m = Omega_m^{-1} L_m B_m^{-1} = D_m^{-1} L_m                                   (P x K),
//   D_m^{-1} = Omega_m^{-1} - a M_m (Omega_m^{-1} L_m)'                              (Woodbury on D_m),
//   Sigma(s)^{-1} = D^{-1} - rho (M S^{-1}) M'                                       (Woodbury on Sigma),
// i.e. with the two thin panels  Left_m = [rho M_m S^{-1} | a M_m],  Right_m = [M_m | Omega_m^{-1} L_m]
//   Sigma(s)^{-1}_ab = [a == b] / omega_a - LeftG_a . RightG_b - [a, b in one shard] LeftA_a . RightA_b.
// Only the inverses B_m^{-1} and S^{-1} are needed (gj.h: no Cholesky), the identity stays unscaled in B_m
// and S, so rho = 0 (LeftG = 0) and rho = 1 (LeftA = 0) need no special case.  Both products are symmetric
// in exact arithmetic; one triangle is stored and mirrored at the read-out, as for Sigmaout.
//
// Every rank forms the panels of ALL g shards from the gathered Lb / wslot of the flush (p K^2 per sample
// against p^2 K for the accumulation), so the sum over the shards needs no collective and every rank feeds
// the same factor bytes to the tiles it owns.  The panel stage (launch_precision_panels: the first three kernels)
// runs once per flush for this file's accumulation and for partial_corr.hip, which scales the panels in place
// behind launch_precision_mean.  Four launches per flush, in stream order (no hand-off
// between blocks, no floating-point atomics, no data-dependent trip count: a NaN state runs through):
//   k_pm_shard   (shard, slot): G_m by v_mfma_f64_16x16x4 over the shard's rows (staged 32 at a time, weighted
//                by 1 / omega), B_m^{-1} in LDS (gj_invert), H_m = B_m^{-1} G_m;
//   k_pm_s       (slot): S = I + rho sum_m H_m in shard order, S^{-1};
//   k_pm_panels  (64 rows of a shard, slot): X = Omega^{-1} L (staged in LDS), M = X B^{-1} and M S^{-1} as
//                MFMA tiles, written into the factor buffer Fb [p][4 KH], KH = round_up(B K, ASM_KC):
//                columns [0, KH) LeftG, [KH, 2 KH) LeftA, [2 KH, 3 KH) RightG, [3 KH, 4 KH) RightA, slot s
//                at s K inside each; the last slot's blocks zero the chunk tail [used, round_up(used, ASM_KC));
//   k_assemble_prec, twice: k_assemble's tile loop with a left and a right panel.  Pass 1 (G half, every
//                tile): Prec -= (1/effsamp) LeftG RightG', diagonal += (1/effsamp) sum_s 1 / omega_a(s).  Pass 2 (A
//                half, the tiles with a same-shard pair): Prec -= (1/effsamp) LeftA RightA' on the same-shard
//                pairs only.  A tile whose rows belong to several shards (P no multiple of 128) needs both
//                coefficients per pair, which one accumulator set cannot hold: hence two passes.
#include "dcfm_internal.h"
#include "gj.h"
#include "tile_linalg.h"

#include <algorithm>

namespace dcfm {

constexpr int PM_ROWS = 32;        // loading rows staged per step of the Gram
constexpr int PM_TPW = 9;          // tiles of a wave: the 36 lower tiles of K = 128 over 4 waves
constexpr int PM_PROWS = 64;       // rows of a k_pm_panels block: 16 per wave
static_assert(precision_tiles(KP_MAX, 0) <= 4 * PM_TPW, "a wave's accumulators hold its tiles");

// doubles of dynamic LDS: the Gram's staged rows, then B (K x K) with gj_invert's panel / mat_apply's columns
static size_t pm_inv_doubles(int K) { return (size_t)K * K + (size_t)K * PREC_PANEL + 2; }
static size_t pm_shard_doubles(int K) {
    const size_t wp = (size_t)(K + 15) / 16 * 16;
    return std::max(PM_ROWS * wp + PM_ROWS, pm_inv_doubles(K));
}
__host__ __device__ constexpr int pm_pitch(int K) { return ((K + 3) & ~3) + 1; }
static size_t pm_panel_doubles(int K) { return 2 * (size_t)PM_PROWS * pm_pitch(K) + PM_PROWS; }

// scr: [slot][shard][2][K][K] = {H_m, B_m^{-1}}
__global__ __launch_bounds__(256) void k_pm_shard(const double *__restrict__ Lb, int LDB,
                                                  const double *__restrict__ wslot, int B, int P, int K, int g,
                                                  double rho, double *scr) {
    extern __shared__ __align__(16) double dyn[];
    const int m = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
    const int wave = t >> 6, lane = t & 63, li = lane & 15, kq = lane >> 4;
    const int nbt = (K + 15) / 16, wp = 16 * nbt, ntl = nbt * (nbt + 1) / 2;
    const double *Lm = Lb + (size_t)m * P * LDB + (size_t)s * K, *wm = wslot + (size_t)m * P * B + s;
    double *Hm = scr + (size_t)(s * g + m) * 2 * K * K, *Bi = Hm + (size_t)K * K;

    // ---- G_m = L' Omega^{-1} L: tile wave + 4 u of the lower triangle
    double *sX = dyn, *sW = dyn + PM_ROWS * wp;
    int cI[PM_TPW], cJ[PM_TPW];
    d4 acc[PM_TPW];
    const int nmine = ntl > wave ? (ntl - wave + 3) / 4 : 0;
#pragma unroll
    for (int u = 0; u < PM_TPW; ++u) {
        int a = 0, b = 0;
        if (u < nmine) tile::tri_pair(wave + 4 * u, a, b);
        cI[u] = 16 * a + li;
        cJ[u] = 16 * b + li;
        acc[u] = d4{0.0, 0.0, 0.0, 0.0};
    }
    for (int r0 = 0; r0 < P; r0 += PM_ROWS) {
        const int nr = min(PM_ROWS, P - r0), nr4 = (nr + 3) & ~3;
        for (int e = t; e < nr4 * wp; e += 256) {
            const int r = e / wp, c = e - r * wp;
            sX[e] = (r < nr && c < K) ? Lm[(size_t)(r0 + r) * LDB + c] : 0.0;
        }
        if (t < nr4) sW[t] = t < nr ? 1.0 / wm[(size_t)(r0 + t) * B] : 0.0;
        __syncthreads();
        for (int r = 0; r < nr4; r += 4) {
            const double *xr = sX + (r + kq) * wp;
            const double wt = sW[r + kq];
#pragma unroll
            for (int u = 0; u < PM_TPW; ++u)
                if (u < nmine) acc[u] = mfma16x16x4(wt * xr[cI[u]], xr[cJ[u]], acc[u]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < PM_TPW; ++u)
        if (u < nmine)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {              // D[row = q + 4 g][col = lane & 15] of the tile
                const int row = cI[u] - li + kq + 4 * gq, col = cJ[u];
                if (row < K && col <= row) {
                    st_agent(Hm + (size_t)row * K + col, acc[u][gq]);
                    st_agent(Hm + (size_t)col * K + row, acc[u][gq]);
                }
            }
    stores_done();

    // ---- B_m^{-1} and H_m = B_m^{-1} G_m (in place: mat_apply reads a column panel whole before it writes it)
    double *A = dyn, *sP = dyn + K * K, *Cc = sP + (K & 1);   // Cc: 16-byte aligned inside the idle panel
    load_shifted(A, K, Hm, K, 1.0 - rho);
    (void)gj_invert(A, K, Cc);
    for (int e = t; e < K * K; e += 256) Bi[e] = A[e];
    mat_apply(A, K, Hm, K, K, Hm, K, sP);
}

// Sinv [slot][K][K] = (I + rho sum_m H_m)^{-1}, the shards in shard order
__global__ __launch_bounds__(256) void k_pm_s(const double *__restrict__ scr, int K, int g, double rho,
                                              double *__restrict__ Sinv) {
    extern __shared__ __align__(16) double dyn[];
    const int s = blockIdx.x, t = threadIdx.x;
    double *A = dyn, *sP = dyn + K * K, *Cc = sP + (K & 1);
    for (int e = t; e < K * K; e += 256) {
        double acc = 0.0;
        for (int m = 0; m < g; ++m) acc += scr[(size_t)(s * g + m) * 2 * K * K + e];
        A[e] = fma(rho, acc, e / K == e % K ? 1.0 : 0.0);
    }
    (void)gj_invert(A, K, Cc);
    for (int e = t; e < K * K; e += 256) Sinv[(size_t)s * K * K + e] = A[e];
}

// one 16-row x K product of a wave: out(i, c) = sum_k X(i, k) M(k, c), X the wave's rows in LDS (pitch), M K x K
// row-major in global memory; f(row of the wave's 16, column, value) takes every entry with column < 16 nbt
template <class F>
__device__ __forceinline__ void pm_rows_times(const double *X, int pitch, const double *__restrict__ M, int K, F &&f) {
    const int lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4;
    const int nbt = (K + 15) / 16, K4 = (K + 3) & ~3;
    for (int jt = 0; jt < nbt; ++jt) {
        const int col = 16 * jt + li;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < K4; k0 += 4) {
            const int kk = k0 + kq;
            const double b = (kk < K && col < K) ? M[(size_t)kk * K + col] : 0.0;
            acc = mfma16x16x4(X[li * pitch + kk], b, acc);
        }
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) f(kq + 4 * gq, col, acc[gq]);
    }
}

__global__ __launch_bounds__(256) void k_pm_panels(const double *__restrict__ Lb, int LDB,
                                                   const double *__restrict__ wslot, int B, int P, int K, int g,
                                                   double rho, const double *__restrict__ scr,
                                                   const double *__restrict__ Sinv, int nslots, int KH,
                                                   double *__restrict__ Fb) {
    extern __shared__ __align__(16) double dyn[];
    const int j0 = blockIdx.x * PM_PROWS, m = blockIdx.y, s = blockIdx.z, t = threadIdx.x, wave = t >> 6;
    const int pitch = pm_pitch(K), K4 = (K + 3) & ~3, LDF = 4 * KH;
    double *sX = dyn, *sM = dyn + PM_PROWS * pitch, *sW = sM + PM_PROWS * pitch;
    const size_t row0 = (size_t)m * P + j0;                  // first global row of the block
    const int nr = min(PM_PROWS, P - j0);
    const double *Bi = scr + ((size_t)(s * g + m) * 2 + 1) * K * K, *Si = Sinv + (size_t)s * K * K;
    double *F0 = Fb + row0 * LDF + (size_t)s * K;

    if (t < PM_PROWS) sW[t] = t < nr ? 1.0 / wslot[(row0 + t) * B + s] : 0.0;
    __syncthreads();
    for (int e = t; e < PM_PROWS * K4; e += 256) {           // X = Omega^{-1} L, zero past the rows and past K
        const int r = e / K4, c = e - r * K4;
        const double v = (r < nr && c < K) ? sW[r] * Lb[(row0 + r) * LDB + (size_t)s * K + c] : 0.0;
        sX[r * pitch + c] = v;
        if (r < nr && c < K) F0[(size_t)r * LDF + 3 * KH + c] = v;                    // RightA
    }
    if (s == nslots - 1) {                                   // the chunk tail of every quarter
        const int used = nslots * K, tail = (used + ASM_KC - 1) / ASM_KC * ASM_KC - used;
        for (int e = t; e < nr * tail * 4; e += 256) {
            const int r = e / (tail * 4), c = e - r * (tail * 4);
            Fb[(row0 + r) * LDF + (size_t)(c / tail) * KH + used + c % tail] = 0.0;
        }
    }
    __syncthreads();
    const double a1 = 1.0 - rho;
    const int w0 = 16 * wave;
    pm_rows_times(sX + w0 * pitch, pitch, Bi, K, [&](int r, int c, double v) {       // M = X B^{-1}
        if (c < K4) sM[(w0 + r) * pitch + c] = c < K ? v : 0.0;
        if (w0 + r < nr && c < K) {
            F0[(size_t)(w0 + r) * LDF + KH + c] = a1 * v;                              // LeftA
            F0[(size_t)(w0 + r) * LDF + 2 * KH + c] = v;                               // RightG
        }
    });
    __syncthreads();
    pm_rows_times(sM + w0 * pitch, pitch, Si, K, [&](int r, int c, double v) {       // M S^{-1}
        if (w0 + r < nr && c < K) F0[(size_t)(w0 + r) * LDF + c] = rho * v;            // LeftG
    });
}

// k_assemble's tile loop with a left (rows) and a right (columns) panel of Fb.  APASS: the A half.
// PC (partial_corr.hip): the panels are scaled by 1 / sqrt(d_a(s)), the sum is the per-sample partial
// correlation: sign +, and the diagonal entry is the count nslots / effsamp itself (G pass; the A pass adds 0)
constexpr int PKC = ASM_KC, PLD = ASM_TILE + 16;
template <bool APASS, bool PC = false>
__global__ __launch_bounds__(256, 2) void k_assemble_prec(Dims d, const double *__restrict__ Fb, int LDF, int offL,
                                                          int offR, int kext, const double *__restrict__ wslot,
                                                          int B, int nslots, double inv_eff,
                                                          const int2 *__restrict__ tiles, int T0,
                                                          double *__restrict__ Prec) {
    __shared__ double As[2][PKC][PLD], Bs[2][PKC][PLD];
    __shared__ int shard_of[2][ASM_TILE];
    const int2 T = tiles[xcd_remap(blockIdx.x, gridDim.x)];
    const int p = d.p;
    if (APASS) {   // no same-shard pair (the rows' shards all lie below the columns'): nothing to add
        const int clast = min(p, T.y * ASM_TILE + ASM_TILE) - 1;
        if ((T.x * ASM_TILE) / d.P > clast / d.P) return;
    }
    double *__restrict__ St = Prec + (size_t)(tri(T.x) - tri(T0) + T.y) * ASM_TILE * ASM_TILE;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    shard_of[t >> 7][t & 127] = ((t < ASM_TILE ? T.x : T.y) * ASM_TILE + (t & 127)) / d.P;
    const int r = lane & 15, q = lane >> 4;
    const int wa = (wave >> 1) * 64, wb = (wave & 1) * 64;
    // global -> LDS: thread t stages row (t >> 1) of both panels, k = 8 (t & 1) .. +7
    const int srow = t >> 1, shalf = t & 1;
    const int ga = T.x * ASM_TILE + srow, gb = T.y * ASM_TILE + srow;
    const bool va = ga < p, vb = gb < p;
    const double *pa = Fb + (size_t)(va ? ga : 0) * LDF + offL + 8 * shalf;
    const double *pb = Fb + (size_t)(vb ? gb : 0) * LDF + offR + 8 * shalf;
    const d2 zero2 = {0.0, 0.0};
    d2 ra[4], rb[4];
    auto gload = [&](int kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = va ? *reinterpret_cast<const d2 *>(pa + kc + 2 * i) : zero2;
            rb[i] = vb ? *reinterpret_cast<const d2 *>(pb + kc + 2 * i) : zero2;
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 8 * shalf + 2 * i;
            As[buf][k][srow] = ra[i].x;
            As[buf][k + 1][srow] = ra[i].y;
            Bs[buf][k][srow] = rb[i].x;
            Bs[buf][k + 1][srow] = rb[i].y;
        }
    };
    d4 acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = d4{0.0, 0.0, 0.0, 0.0};
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kc = 0, buf = 0; kc < kext; kc += PKC, buf ^= 1) {
        const bool more = kc + PKC < kext;
        if (more) gload(kc + PKC);
        const int nk4 = min(PKC, kext - kc);   // k extent of this chunk (a multiple of 4)
#pragma unroll
        for (int s4 = 0; s4 < PKC / 4; ++s4) {
            if (4 * s4 >= nk4) break;            // block-uniform: the last chunk may be partial
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = As[buf][4 * s4 + q][wa + 16 * u + r];
#pragma unroll
            for (int v = 0; v < 4; ++v) b[v] = Bs[buf][4 * s4 + q][wb + 16 * v + r];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = mfma16x16x4(a[u], b[v], acc[u][v]);
        }
        if (more) lstore(buf ^ 1);
        __syncthreads();
    }
    // epilogue: lower-triangle read-modify-write of the tile; the strict upper part of a diagonal tile and
    // the rows past p stay zero (as in Sigma)
    const int a0 = T.x * ASM_TILE + wa, b0 = T.y * ASM_TILE + wb;
    int sb[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) sb[v] = shard_of[1][wb + 16 * v + r];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int a = a0 + 16 * u + q + 4 * g;
            const int sa = shard_of[0][wa + 16 * u + q + 4 * g];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int b = b0 + 16 * v + r;
                if (a < p && b <= a) {
                    double val = (PC ? inv_eff : -inv_eff) * acc[u][v][g];
                    if (APASS && sb[v] != sa) val = 0.0;
                    if (PC && a == b) val = APASS ? 0.0 : (double)nslots * inv_eff;
                    if (!PC && !APASS && a == b) {     // sum_s 1 / omega_a(s), the batch's slots in slot order
                        double ps = 0.0;
                        for (int s = 0; s < nslots; ++s) ps += 1.0 / wslot[(size_t)a * B + s];
                        val = fma(ps, inv_eff, val);
                    }
                    double *ptr = &St[sig_tile_off(u, v, g, wave, lane)];
                    __builtin_nontemporal_store(__builtin_nontemporal_load(ptr) + val, ptr);
                }
            }
        }
}

size_t precision_mean_scratch_doubles(int g, int K, int B) { return (size_t)(2 * g + 1) * B * K * K; }

// the footprints at K = 128 pass the default limit of dynamic LDS; the attribute belongs to the kernel
hipError_t precision_mean_setup() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_pm_shard),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)(pm_shard_doubles(KP_MAX) * sizeof(double)));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_pm_s), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(pm_inv_doubles(KP_MAX) * sizeof(double)));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_pm_panels), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(pm_panel_doubles(KP_MAX) * sizeof(double)));
    return e;
}

void launch_precision_panels(const Dims &d, const Bufs &b, const PrecMean &pm, const double *Lb, const double *wslot,
                             int nslots, int B, hipStream_t s) {
    if (nslots == 0) return;
    const int K = d.K, g = d.g, KH = pm.KH;
    double *scr = pm.pscr, *Sinv = scr + (size_t)2 * g * B * K * K;
    hipLaunchKernelGGL(k_pm_shard, dim3(g, nslots), dim3(256), pm_shard_doubles(K) * sizeof(double), s, Lb, b.LDB,
                       wslot, B, d.P, K, g, d.rho, scr);
    hipLaunchKernelGGL(k_pm_s, dim3(nslots), dim3(256), pm_inv_doubles(K) * sizeof(double), s, scr, K, g, d.rho, Sinv);
    hipLaunchKernelGGL(k_pm_panels, dim3(cdiv(d.P, PM_PROWS), g, nslots), dim3(256),
                       pm_panel_doubles(K) * sizeof(double), s, Lb, b.LDB, wslot, B, d.P, K, g, d.rho, scr, Sinv,
                       nslots, KH, pm.pfac);
}

void launch_precision_mean(const Dims &d, const Bufs &b, const PrecMean &pm, const double *wslot, int nslots, int B,
                           double inv_eff, hipStream_t s) {
    if (nslots == 0 || b.ntiles == 0) return;
    const int K = d.K, KH = pm.KH, LDF = 4 * KH;
    const int kext = (nslots * K + 3) & ~3;
    hipLaunchKernelGGL(k_assemble_prec<false>, dim3(b.ntiles), dim3(256), 0, s, d, pm.pfac, LDF, 0, 2 * KH, kext,
                       wslot, B, nslots, inv_eff, b.tiles, b.T0, pm.Prec);
    hipLaunchKernelGGL(k_assemble_prec<true>, dim3(b.ntiles), dim3(256), 0, s, d, pm.pfac, LDF, KH, 3 * KH, kext,
                       wslot, B, nslots, inv_eff, b.tiles, b.T0, pm.Prec);
}

void launch_pc_mean(const Dims &d, const Bufs &b, const PrecMean &pm, int nslots, double inv_eff, double *PC,
                    hipStream_t s) {
    if (nslots == 0 || b.ntiles == 0) return;
    const int KH = pm.KH, LDF = 4 * KH, kext = (nslots * d.K + 3) & ~3;
    hipLaunchKernelGGL((k_assemble_prec<false, true>), dim3(b.ntiles), dim3(256), 0, s, d, pm.pfac, LDF, 0, 2 * KH, kext,
                       nullptr, 0, nslots, inv_eff, b.tiles, b.T0, PC);
    hipLaunchKernelGGL((k_assemble_prec<true, true>), dim3(b.ntiles), dim3(256), 0, s, d, pm.pfac, LDF, KH, 3 * KH, kext,
                       nullptr, 0, nslots, inv_eff, b.tiles, b.T0, PC);
}

}  // namespace dcfm
