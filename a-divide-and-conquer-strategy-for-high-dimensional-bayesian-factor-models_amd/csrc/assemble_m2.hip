// Second moment of the per-sample covariance (DCFM_FLAG_SIGMA_M2): next to the mean Sigmaout,
//   Sigma2[a][b] += (1/effsamp) sum_s ( c_ab Lambda_a^(s) . Lambda_b^(s) + [a==b] omega_a^(s) )^2
// over the saved samples s of a batch (dc:182-192 per sample, squared element-wise), c_ab = 1
// inside a shard and rho across.  k_assemble cannot give it: it runs all samples of a batch
// along one k extent, so the per-sample product never exists.
#include "slot_tiles.h"

namespace dcfm {
using namespace slot;

// k_assemble_m2: the per-slot tile loop of slot_tiles.h over Lb into Sigma2, nph = 1.  Its own: cross-shard tiles
// stage the row panel scaled by rho (t = rho L_a.L_b, no diagonal), so their per-slot update is the 32 fma alone;
// the other tiles take the per-pair coefficient and, on the diagonal, this sample's omega in the fold.
__global__ __launch_bounds__(THREADS) void k_assemble_m2(Dims d, const double *__restrict__ Lb, int LDB,
                                                          int nslots, const double *__restrict__ wslot, int B,
                                                          double inv_eff, const int2 *__restrict__ tiles,
                                                          int T0, double *__restrict__ Sig2) {
    __shared__ Panel As, Bs;
    __shared__ int shard_of[2][ASM_TILE];      // shard of the tile's rows / columns
    const Tile g(d, tiles, T0, shard_of);
    const Rows R(g, d);
    const int p = d.p, K = d.K;
    const double *prow[4];
    R.pointers(prow, Lb, Lb, LDB);
    const double sA = g.cross ? d.rho : 1.0;   // row-panel scale while staging
    double rg[8];
    auto gload = [&](int s, int, int c) { R.load(rg, prow, (size_t)s * K + KC * c, c, K); };
    auto lstore = [&](int buf, int) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < 4) As[buf][R.k(i)][R.row(i)] = sA * rg[i];
            else Bs[buf][R.k(i)][R.row(i)] = rg[i];
        }
    };
    d4 acc2[2][4];
    zero(acc2);
    auto fold = [&](int s, const d4 (&acc)[2][4]) {
        if (g.cross) return each([&](int u, int v, int e) { acc2[u][v][e] = fma(acc[u][v][e], acc[u][v][e], acc2[u][v][e]); });
        double dg[2][4];    // this sample's omega of the thread's rows, on a diagonal tile
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int a = g.a0() + 16 * (j >> 2) + g.q + 4 * (j & 3);
            dg[j >> 2][j & 3] = (g.diag && a < p) ? wslot[(size_t)a * B + s] : 0.0;
        }
        pairs(g, shard_of, d.rho, acc, [&](int u, int v, int e, int, bool eq, double tv) {
            if (eq) tv += dg[u][e];
            acc2[u][v][e] = fma(tv, tv, acc2[u][v][e]);
        });
    };
    auto none = [](int, int, int) {};
    loop<1>(g, As, Bs, K, nslots, 1, gload, lstore, none, none, fold);
    add_tile(g, Sig2 + g.off, p, inv_eff, acc2);
}

void launch_assemble_m2(const Dims &d, const Bufs &b, const double *Lb, const double *wslot, int nslots, int B,
                        double inv_eff, hipStream_t s) {
    if (b.ntiles == 0 || nslots == 0) return;
    hipLaunchKernelGGL(k_assemble_m2, dim3(b.ntiles), dim3(THREADS), 0, s, d, Lb, b.LDB, nslots, wslot, B,
                       inv_eff, b.tiles, b.T0, b.Sigma2);
}

}  // namespace dcfm
