// Posterior mean and second moment of the partial correlations (DCFM_FLAG_PARTIAL_CORR): next to Sigmaout,
//   PC [a][b] += (1/effsamp) sum_s R(s)_ab,    PC2[a][b] += (1/effsamp) sum_s R(s)_ab^2,
//   R(s)_ab = -Theta(s)_ab / sqrt(d_a(s) d_b(s))  (a != b),  R(s)_aa = 1,  Theta(s) = Sigma(s)^{-1},  d_a = Theta_aa,
// over the saved samples s of a batch, on the assembly stream behind the precision mean.  R(s) is not linear in
// Theta(s), so neither moment follows from the precision mean: both need the per-sample matrix.
//
// The four thin panels of Theta(s) are those of precision_mean.hip (LeftG, LeftA, RightG, RightA; slot s at
// columns s K of each quarter of the factor buffer, written once per flush by the shared panel stage):
//   d_a(s)  = 1 / omega_a(s) - LeftG_a . RightG_a - LeftA_a . RightA_a,
//   R(s)_ab = ( LeftG_a . RightG_b + [a, b in one shard] LeftA_a . RightA_b ) / sqrt(d_a d_b)     (a != b).
// Three stages per flush, in stream order (no hand-off between blocks, no floating-point atomics, no
// data-dependent trip count or branch on a value: a non-positive or non-finite d gives NaN, which runs through):
//   k_pc_scale        (row, slot): d_a(s) by two K-length dot products, k ascending; the row's four panel
//                     pieces of the slot times 1 / sqrt(d_a(s)), IN PLACE: the precision-mean passes of the flush
//                     have read the buffer by then and the next flush rewrites it (no second p x 4 KH buffer);
//                     the chunk tail stays zero;
//   k_assemble_prec<., PC>, twice (precision_mean.hip): the mean, all slots along one k extent, G pass and A pass;
//   k_assemble_pc_m2  the second moment: per 128 x 128 lower tile the slots run one after the other, as in
//                     k_assemble_m2, but a slot's k extent is K (1 + the shards common to the tile's rows and
//                     columns): the G half over all pairs, then per common shard sigma the A half staged with
//                     the rows and columns of the other shards zeroed, into the same product accumulators.  So
//                     the per-pair coefficient [a, b in one shard] is inside t before t is squared, exactly
//                     (a zeroed row adds +0 products), without a second accumulator set.
// The diagonal of both accumulators gets the count itself, nslots / effsamp per flush (R(s)_aa = 1, not a computed
// 1 - rounding).  A sum of such terms over several flushes can still round (0.4 + 0.4 + 0.4 != 3 / 2.5), so the
// read-out writes the diagonal from the handle's own count: saved / effsamp for both moments, 0 for the standard
// deviation (sigma_out.hip, k_sigma_pack's dset).
#include "dcfm_internal.h"
#include "linalg.h"

namespace dcfm {

constexpr int PCS_LANES = 16;      // lanes of a (row, slot) group of k_pc_scale: 16 groups per block, 4 per wave

// Fb [p][4 KH]: the flush's panels, scaled in place.  Every lane of a group forms d itself (the group's loads
// are broadcasts), so the scale needs no exchange; a lane's stores depend on every load of its wave's groups
// through d, and the groups of other waves own other (row, slot) pieces
__global__ __launch_bounds__(256) void k_pc_scale(double *Fb, int KH, const double *__restrict__ wslot, int B, int p,
                                                  int K, int nslots) {
    const long long gi = (long long)blockIdx.x * (256 / PCS_LANES) + (threadIdx.x / PCS_LANES);
    const int l = threadIdx.x % PCS_LANES;
    if (gi >= (long long)p * nslots) return;
    const int a = (int)(gi / nslots), s = (int)(gi - (long long)a * nslots);
    double *F = Fb + (size_t)a * 4 * KH + (size_t)s * K;
    double dg = 0.0, da = 0.0;
    for (int k = 0; k < K; ++k) dg = fma(F[k], F[2 * (size_t)KH + k], dg);
    for (int k = 0; k < K; ++k) da = fma(F[(size_t)KH + k], F[3 * (size_t)KH + k], da);
    const double dd = 1.0 / wslot[(size_t)a * B + s] - dg - da;
    const double sc = 1.0 / sqrt(dd);
    __builtin_amdgcn_wave_barrier();
    for (int k = l; k < K; k += PCS_LANES)
#pragma unroll
        for (int h = 0; h < 4; ++h) F[h * (size_t)KH + k] *= sc;
}

// ============================================================================
// k_assemble_pc_m2: k_assemble_m2's tile list, XCD remap, block-sharding, wave tile (8 waves, each 32 x 64:
// 64 product and 64 square accumulator VGPRs) and tile-packed layout, into PC2.  The operands are two distinct
// panels of the scaled factor buffer: the tile's rows from the Left quarters, its columns from the Right ones.
// A slot runs nph = 1 + ncommon phases of nch chunks: phase 0 the G quarters, phase 1 + i the A quarters with
// every row of both panels outside shard sig0 + i staged as zero.  A slot starts at column s K of a quarter
// (8-byte aligned only) and ends inside a k-step unless 4 | K: staging is predicated on k < K, as in k_assemble_m2.
// After the slot's last chunk t = the product, 1 on the diagonal, acc2 = fma(t, t, acc2), the product restarts.
// ============================================================================
constexpr int CKC = ASM_KC, CLD = ASM_TILE + 16, PC2_THREADS = 512;

__global__ __launch_bounds__(PC2_THREADS) void k_assemble_pc_m2(Dims d, const double *__restrict__ Fb, int KH,
                                                                int nslots, double inv_eff,
                                                                const int2 *__restrict__ tiles, int T0,
                                                                double *__restrict__ PC2) {
    __shared__ double As[2][CKC][CLD], Bs[2][CKC][CLD];
    const int2 T = tiles[xcd_remap(blockIdx.x, gridDim.x)];
    double *__restrict__ St = PC2 + (size_t)(tri(T.x) - tri(T0) + T.y) * ASM_TILE * ASM_TILE;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int r = lane & 15, q = lane >> 4;
    const int p = d.p, K = d.K;
    const size_t LDF = 4 * (size_t)KH;
    const int w4 = wave >> 1, u0 = 2 * (wave & 1);           // k_assemble's wave and first 16-row tile
    const int wa = (w4 >> 1) * 64 + 16 * u0, wb = (w4 & 1) * 64;
    // the rows' shards are sig0 .. and the columns' end at clast / P <= the rows' last (T.y <= T.x): the
    // shards present on both sides are sig0 .. clast / P (none on a pure cross-shard tile)
    const int clast = min(p, T.y * ASM_TILE + ASM_TILE) - 1;
    const int sig0 = (T.x * ASM_TILE) / d.P;
    const int nph = 1 + max(0, clast / d.P - sig0 + 1);
    const bool diag = T.x == T.y;
    // global -> LDS as k_assemble_m2: value i of thread t is column (t & 7) + 8 (i & 1) of row
    // (t >> 3) + 64 (i >> 1) of [row panel | column panel]
    const int k8 = t & 7, rsub = t >> 3;
    const double *prow[4];
    bool vrow[4];
    int shr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int grow = (j < 2 ? T.x : T.y) * ASM_TILE + ((rsub + 64 * j) & 127);
        vrow[j] = grow < p;
        shr[j] = grow / d.P;
        prow[j] = Fb + (size_t)(vrow[j] ? grow : 0) * LDF + (j < 2 ? 0 : 2 * (size_t)KH) + k8;
    }
    const int K4 = (K + 3) & ~3, nch = (K4 + CKC - 1) / CKC, total = nslots * nph * nch;
    double rg[8];
    auto gload = [&](int s, int ph, int c) {   // chunk c of phase ph of slot s: columns s*K + 16 c + [0, 16), those < K
        const size_t col = (ph ? (size_t)KH : 0) + (size_t)s * K + CKC * c;
        const int kleft = K - CKC * c - k8;    // this thread's columns k8, k8 + 8 are valid if > 0, > 8
        const int sig = sig0 + ph - 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = vrow[i >> 1] && 8 * (i & 1) < kleft && (ph == 0 || shr[i >> 1] == sig);
            rg[i] = ok ? prow[i >> 1][col + 8 * (i & 1)] : 0.0;
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k8 + 8 * (i & 1), row = (rsub + 64 * (i >> 1)) & 127;
            if (i < 4) As[buf][k][row] = rg[i];
            else Bs[buf][k][row] = rg[i];
        }
    };
    d4 acc[2][4], acc2[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = acc2[u][v] = d4{0.0, 0.0, 0.0, 0.0};
    if (total > 0) {
        gload(0, 0, 0);
        lstore(0);
    }
    __syncthreads();
    const int a0 = T.x * ASM_TILE + wa, b0 = T.y * ASM_TILE + wb;
    for (int i = 0, s = 0, ph = 0, c = 0, buf = 0; i < total; ++i, buf ^= 1) {
        const bool more = i + 1 < total;
        const bool last_chunk = c == nch - 1, last_phase = ph == nph - 1;
        const int cn = last_chunk ? 0 : c + 1;
        const int phn = last_chunk ? (last_phase ? 0 : ph + 1) : ph;
        const int sn = (last_chunk && last_phase) ? s + 1 : s;
        if (more) gload(sn, phn, cn);
        const int nk4 = min(CKC, K4 - CKC * c);   // k extent of this chunk (a multiple of 4)
#pragma unroll
        for (int s4 = 0; s4 < CKC / 4; ++s4) {
            if (4 * s4 >= nk4) break;            // block-uniform
            double a[2], b[4];
#pragma unroll
            for (int u = 0; u < 2; ++u) a[u] = As[buf][4 * s4 + q][wa + 16 * u + r];
#pragma unroll
            for (int v = 0; v < 4; ++v) b[v] = Bs[buf][4 * s4 + q][wb + 16 * v + r];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = mfma16x16x4(a[u], b[v], acc[u][v]);
        }
        if (last_chunk && last_phase) {   // the slot's R(s) tile is complete: square it into acc2, restart the product
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int a = a0 + 16 * u + q + 4 * g;
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int b = b0 + 16 * v + r;
                        const double tv = (diag && a == b) ? 1.0 : acc[u][v][g];
                        acc2[u][v][g] = fma(tv, tv, acc2[u][v][g]);
                    }
                }
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = d4{0.0, 0.0, 0.0, 0.0};
        }
        if (more) lstore(buf ^ 1);
        __syncthreads();
        s = sn;
        ph = phn;
        c = cn;
    }
    // epilogue: PC2 tile += acc2 / effsamp, the wave's (u, v, h) slices as 16-byte accesses; the strict upper
    // part of a diagonal tile and the rows past p stay zero (as in Sigma)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                d2 *ptr = reinterpret_cast<d2 *>(St + sig_tile_off(u0 + u, v, 2 * h, w4, lane));
                const int b = b0 + 16 * v + r, a = a0 + 16 * u + q + 8 * h;
                d2 o = __builtin_nontemporal_load(ptr);
                o.x += (a < p && b <= a) ? inv_eff * acc2[u][v][2 * h] : 0.0;
                o.y += (a + 4 < p && b <= a + 4) ? inv_eff * acc2[u][v][2 * h + 1] : 0.0;
                __builtin_nontemporal_store(o, ptr);
            }
}

void launch_partial_corr(const Dims &d, const Bufs &b, const PrecMean &pm, const PartialCorr &pc, const double *wslot,
                         int nslots, int B, double inv_eff, hipStream_t s) {
    if (nslots == 0) return;
    const long long groups = (long long)d.p * nslots;
    const int per = 256 / PCS_LANES;
    hipLaunchKernelGGL(k_pc_scale, dim3((unsigned)((groups + per - 1) / per)), dim3(256), 0, s, pm.pfac, pm.KH, wslot, B,
                       d.p, d.K, nslots);
    launch_pc_mean(d, b, pm, nslots, inv_eff, pc.PC, s);
    if (b.ntiles == 0) return;
    hipLaunchKernelGGL(k_assemble_pc_m2, dim3(b.ntiles), dim3(PC2_THREADS), 0, s, d, pm.pfac, pm.KH, nslots, inv_eff,
                       b.tiles, b.T0, pc.PC2);
}

}  // namespace dcfm
