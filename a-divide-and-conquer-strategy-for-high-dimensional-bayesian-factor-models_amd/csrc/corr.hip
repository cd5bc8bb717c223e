// Posterior mean and second moment of the marginal correlations, and of the communalities (DCFM_FLAG_CORR):
// next to Sigmaout,
//   C [a][b] += (1/effsamp) sum_s R(s)_ab,    C2[a][b] += (1/effsamp) sum_s R(s)_ab^2,
//   H [a]    += (1/effsamp) sum_s h_a(s),     H2[a]    += (1/effsamp) sum_s h_a(s)^2,
// over the saved samples s of a batch, with (dc:182-192 per sample; c_ab = 1 inside a shard, rho across)
//   v_a(s)  = sum_k Lambda_ak(s)^2 + omega_a(s)                 the diagonal of Sigma(s),
//   s_a(s)  = 1 / sqrt(v_a(s)),
//   R(s)_ab = c_ab s_a s_b Lambda_a(s) . Lambda_b(s)  (a != b),  R(s)_aa = 1,
//   h_a(s)  = (sum_k Lambda_ak(s)^2) / v_a(s)                   the communality.
// R(s) is Sigma(s) with its rows and columns scaled, so it needs no inversion, no panels and no K x K scratch:
// two stages per flush, in stream order (no hand-off between blocks, no floating-point atomics, no branch or
// trip count that depends on a value: a non-finite or non-positive v gives NaN, which runs through):
//   k_corr_scale  one 16-lane group per row: cscale[a][s] = s_a(s) for the batch's slots, and the row's H, H2;
//   k_corr        the per-slot tile loop (slot_tiles.h) over Lb with the scale applied while staging: the row panel times
//                 s_a(s) (times rho on a cross-shard tile), the column panel times s_b(s).  Lb is only read.
// Every rank holds the gathered Lb / wslot of all shards: it computes all p scales and communalities (identical
// on every rank) and the tiles it owns.
#include "slot_tiles.h"

namespace dcfm {
using namespace slot;

constexpr int CS_LANES = 16;       // lanes of a row's group in k_corr_scale: 16 groups per block, 4 per wave

// Lane l of row a's group takes slots l, l + 16, ...: sum_k Lambda_ak^2 as one k-ascending fma chain, v, the
// scale.  The row's communalities are then added slot by slot in ascending order, every lane of the group running
// the same chain on values passed round by shuffle (the group's lanes are always all active: the round count
// depends on nslots alone), lane 0 stores.
__global__ __launch_bounds__(256) void k_corr_scale(const double *__restrict__ Lb, int LDB,
                                                    const double *__restrict__ wslot, int B, int p, int K, int nslots,
                                                    double inv_eff, double *__restrict__ cscale,
                                                    double *__restrict__ H, double *__restrict__ H2) {
    const int a = blockIdx.x * (256 / CS_LANES) + threadIdx.x / CS_LANES;
    const int l = threadIdx.x % CS_LANES;
    const bool row = a < p;
    const size_t ar = row ? a : 0;     // rows past p run along on row 0 and store nothing (the shuffles stay full)
    const double *L = Lb + ar * LDB;
    double h1 = H[ar], h2 = H2[ar];
    for (int s0 = 0; s0 < nslots; s0 += CS_LANES) {
        const int s = s0 + l;
        const bool ok = s < nslots;
        const double *Ls = L + (size_t)(ok ? s : 0) * K;
        double ss = 0.0;
        for (int k = 0; k < K; ++k) ss = fma(Ls[k], Ls[k], ss);
        const double v = ss + wslot[ar * B + (ok ? s : 0)];
        const double hv = ss / v;
        if (row && ok) cscale[ar * B + s] = 1.0 / sqrt(v);
        const int nj = min(CS_LANES, nslots - s0);
        for (int j = 0; j < nj; ++j) {
            const double hj = __shfl(hv, j, CS_LANES);
            const double t = inv_eff * hj;
            h1 += t;
            h2 = fma(t, hj, h2);
        }
    }
    if (row && l == 0) {
        H[a] = h1;
        H2[a] = h2;
    }
}

// k_corr: the per-slot tile loop of slot_tiles.h over Lb into C and C2 at once (the panels are read once per
// flush), nph = 1.  Its own: each staged value times its row's scale of that slot (cscale, through the Ss ring in
// LDS); after the slot's last chunk t is the product (times c_ab per pair on a mixed tile, 1 on the diagonal):
// acc1 += t, acc2 = fma(t, t, acc2).  64 product + 64 mean + 64 square accumulator VGPRs.  The read-out writes the
// diagonal from the saved count (sigma_out.hip), so what lands on it here (nslots / effsamp per flush) is never read.
__global__ __launch_bounds__(THREADS) void k_corr(Dims d, const double *__restrict__ Lb, int LDB, int nslots,
                                                  const double *__restrict__ cscale, int B, double inv_eff,
                                                  const int2 *__restrict__ tiles, int T0,
                                                  double *__restrict__ C1, double *__restrict__ C2) {
    __shared__ Panel As, Bs;
    __shared__ int shard_of[2][ASM_TILE];      // shard of the tile's rows / columns
    __shared__ double Ss[3][2 * ASM_TILE];     // scales of the tile's rows | columns, slot s in Ss[s % 3]
    const Tile g(d, tiles, T0, shard_of);
    const Rows R(g, d);
    const int t = g.t, p = d.p, K = d.K;
    const double *prow[4];
    R.pointers(prow, Lb, Lb, LDB);
    const double sA = g.cross ? d.rho : 1.0;   // on the row panel, beside its scale
    // the scales go through LDS too (a thread's four rows' scales in registers do not fit beside three
    // accumulator sets): thread t < 256 fetches the scale of row t of [row panel | column panel], zero past p,
    // times rho on the row panel of a cross-shard tile; Ss holds three consecutive slots, slot s + 2 is written
    // while slot s's first chunk is multiplied and first read, behind a barrier, when slot s + 1 is staged
    const int srow = (t < ASM_TILE ? g.T.x : g.T.y) * ASM_TILE + (t & 127);
    auto sload = [&](int s) {
        return (t < 2 * ASM_TILE && srow < p && s < nslots) ? (t < ASM_TILE ? sA : 1.0) * cscale[(size_t)srow * B + s] : 0.0;
    };
    double rg[8], sreg = 0.0;
    auto gload = [&](int s, int, int c) { R.load(rg, prow, (size_t)s * K + KC * c, c, K); };
    auto lstore = [&](int buf, int s) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            (i < 4 ? As : Bs)[buf][R.k(i)][R.row(i)] = Ss[s % 3][(i < 4 ? 0 : ASM_TILE) + R.row(i)] * rg[i];
    };
    auto head = [&](int s, int, int c) {
        if (c == 0) sreg = sload(s + 2);       // block-uniform
    };
    auto tail = [&](int s, int, int c) {
        if (c == 0 && t < 2 * ASM_TILE) Ss[(s + 2) % 3][t] = sreg;
    };
    d4 acc1[2][4], acc2[2][4];
    zero(acc1);
    zero(acc2);
    auto fold = [&](int, const d4 (&acc)[2][4]) {
        if (g.cross)
            return each([&](int u, int v, int e) {
                acc1[u][v][e] += acc[u][v][e];
                acc2[u][v][e] = fma(acc[u][v][e], acc[u][v][e], acc2[u][v][e]);
            });
        pairs(g, shard_of, d.rho, acc, [&](int u, int v, int e, int, bool eq, double tv) {
            if (g.diag && eq) tv = 1.0;
            acc1[u][v][e] += tv;
            acc2[u][v][e] = fma(tv, tv, acc2[u][v][e]);
        });
    };
    if (t < 2 * ASM_TILE) {
        Ss[0][t] = sload(0);
        Ss[1][t] = sload(1);
    }
    __syncthreads();
    loop<1>(g, As, Bs, K, nslots, 1, gload, lstore, head, tail, fold);
    add_tile(g, C1 + g.off, p, inv_eff, acc1);
    add_tile(g, C2 + g.off, p, inv_eff, acc2);
}

void launch_corr(const Dims &d, const Bufs &b, const Corr &cr, const double *Lb, const double *wslot, int nslots,
                 int B, double inv_eff, hipStream_t s) {
    if (nslots == 0) return;
    const int per = 256 / CS_LANES;
    hipLaunchKernelGGL(k_corr_scale, dim3((d.p + per - 1) / per), dim3(256), 0, s, Lb, b.LDB, wslot, B, d.p, d.K,
                       nslots, inv_eff, cr.cscale, cr.H, cr.H2);
    if (b.ntiles == 0) return;
    hipLaunchKernelGGL(k_corr, dim3(b.ntiles), dim3(THREADS), 0, s, d, Lb, b.LDB, nslots, cr.cscale, B, inv_eff,
                       b.tiles, b.T0, cr.C, cr.C2);
}

}  // namespace dcfm
