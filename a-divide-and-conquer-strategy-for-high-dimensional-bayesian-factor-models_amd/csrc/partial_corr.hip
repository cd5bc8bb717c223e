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
#include "slot_tiles.h"

namespace dcfm {
using namespace slot;

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

// k_assemble_pc_m2: the per-slot tile loop of slot_tiles.h into PC2.  Its own: the operands are two distinct panels
// of the scaled factor buffer, the tile's rows from the Left quarters, its columns from the Right ones; a slot runs
// nph = 1 + ncommon phases: phase 0 the G quarters, phase 1 + i the A quarters with every row of both panels outside
// shard sig0 + i staged as zero; the fold takes 1 on the diagonal.
__global__ __launch_bounds__(THREADS) void k_assemble_pc_m2(Dims d, const double *__restrict__ Fb, int KH, int nslots,
                                                            double inv_eff, const int2 *__restrict__ tiles, int T0,
                                                            double *__restrict__ PC2) {
    __shared__ Panel As, Bs;
    const Tile g(d, tiles, T0);
    const Rows R(g, d);
    const int p = d.p, K = d.K;
    // the rows' shards are sig0 .. and the columns' end at clast / P <= the rows' last (T.y <= T.x): the
    // shards present on both sides are sig0 .. clast / P (none on a pure cross-shard tile)
    const int sig0 = (g.T.x * ASM_TILE) / d.P;
    const int nph = 1 + max(0, g.clast / d.P - sig0 + 1);
    const double *prow[4];
    R.pointers(prow, Fb, Fb + 2 * (size_t)KH, 4 * (size_t)KH);
    double rg[8];
    auto gload = [&](int s, int ph, int c) {   // columns s*K + 16 c + [0, 16) of the phase's quarters, those < K
        const size_t col = (ph ? (size_t)KH : 0) + (size_t)s * K + KC * c;
        const int sig = sig0 + ph - 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = R.has(i, c, K) && (ph == 0 || R.shard[i >> 1] == sig);
            rg[i] = ok ? prow[i >> 1][col + 8 * (i & 1)] : 0.0;
        }
    };
    auto lstore = [&](int buf, int) {
#pragma unroll
        for (int i = 0; i < 8; ++i) (i < 4 ? As : Bs)[buf][R.k(i)][R.row(i)] = rg[i];
    };
    d4 acc2[2][4];
    zero(acc2);
    auto fold = [&](int, const d4 (&acc)[2][4]) {
        each([&](int u, int v, int e) {
            const int a = g.a0() + 16 * u + g.q + 4 * e, b = g.b0() + 16 * v + g.r;
            const double tv = (g.diag && a == b) ? 1.0 : acc[u][v][e];
            acc2[u][v][e] = fma(tv, tv, acc2[u][v][e]);
        });
    };
    auto none = [](int, int, int) {};
    loop<0>(g, As, Bs, K, nslots, nph, gload, lstore, none, none, fold);
    add_tile(g, PC2 + g.off, p, inv_eff, acc2);
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
    hipLaunchKernelGGL(k_assemble_pc_m2, dim3(b.ntiles), dim3(THREADS), 0, s, d, pm.pfac, pm.KH, nslots, inv_eff,
                       b.tiles, b.T0, pc.PC2);
}

}  // namespace dcfm
