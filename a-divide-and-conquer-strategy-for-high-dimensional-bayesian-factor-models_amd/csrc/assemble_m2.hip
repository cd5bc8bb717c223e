// Second moment of the per-sample covariance (DCFM_FLAG_SIGMA_M2): next to the mean Sigmaout,
//   Sigma2[a][b] += (1/effsamp) sum_s ( c_ab Lambda_a^(s) . Lambda_b^(s) + [a==b] omega_a^(s) )^2
// over the saved samples s of a batch (dc:182-192 per sample, squared element-wise), c_ab = 1
// inside a shard and rho across.  k_assemble cannot give it: it runs all samples of a batch
// along one k extent, so the per-sample product never exists.
#include "dcfm_internal.h"
#include "linalg.h"

namespace dcfm {

// ============================================================================
// k_assemble_m2: same tile list, XCD remap, block-sharding and tile-packed layout (sig_tile_off)
// as k_assemble, into Sigma2.  Per 128x128 lower-triangle tile the samples (slots) of the batch
// run one after the other: the slot's K columns of Lb go through LDS in chunks of 16, zero-padded
// to the MFMA k-step (a slot starts at column s*K: 8-byte aligned only, and ends inside a k-step
// unless 4 | K, so the chunk is staged with 8-byte loads predicated on k < K and never touches the
// neighbour slot's columns); after the slot's last chunk the product t is squared into the running
// accumulator, fma(t, t, acc2), and the product accumulators restart from zero.  One
// read-modify-write of the Sigma2 tile at the end of the batch.
// 8 waves, each 32x64 = 2x4 tiles of v_mfma_f64_16x16x4: 64 accumulator VGPRs for the product and
// 64 for the square (a 64x64 wave tile would need 128 + 128 before operands: one wave per SIMD).
// Wave w covers rows 32 (w & 1) .. + 31 of k_assemble's wave w >> 1, so the Sigma2 tile has the
// layout of the Sigma tile.  Cross-shard tiles stage the row panel scaled by rho (t = rho L_a.L_b,
// no diagonal): their per-slot update is the 32 fma alone.
// ============================================================================
constexpr int MKC = ASM_KC, MLD = ASM_TILE + 16, M2_THREADS = 512;

__global__ __launch_bounds__(M2_THREADS) void k_assemble_m2(Dims d, const double *__restrict__ Lb, int LDB,
                                                             int nslots, const double *__restrict__ wslot, int B,
                                                             double inv_eff, const int2 *__restrict__ tiles,
                                                             int T0, double *__restrict__ Sig2) {
    __shared__ double As[2][MKC][MLD], Bs[2][MKC][MLD];
    __shared__ int shard_of[2][ASM_TILE];      // shard of the tile's rows / columns
    const int2 T = tiles[xcd_remap(blockIdx.x, gridDim.x)];
    double *__restrict__ St = Sig2 + (size_t)(tri(T.x) - tri(T0) + T.y) * ASM_TILE * ASM_TILE;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (t < 2 * ASM_TILE) shard_of[t >> 7][t & 127] = ((t < ASM_TILE ? T.x : T.y) * ASM_TILE + (t & 127)) / d.P;
    const int r = lane & 15, q = lane >> 4;
    const int p = d.p, K = d.K;
    const int w4 = wave >> 1, u0 = 2 * (wave & 1);           // k_assemble's wave and first 16-row tile
    const int wa = (w4 >> 1) * 64 + 16 * u0, wb = (w4 & 1) * 64;
    const int clast = min(p, T.y * ASM_TILE + ASM_TILE) - 1;
    const bool cross = (T.x * ASM_TILE) / d.P > clast / d.P;  // as k_assemble: coef = rho everywhere
    const bool diag = T.x == T.y;
    // global -> LDS: a chunk is 16 columns of the 256 rows of both panels, 8 values per thread.
    // Lanes 8 j .. 8 j + 7 read 8 consecutive columns of one row, so a wave's load touches 8 rows (8 to
    // 16 cache lines; one row per lane pair touched 64 and left the staging bound by the L1's line rate):
    // value i of thread t is column (t & 7) + 8 (i & 1) of row (t >> 3) + 64 (i >> 1) of [row panel | column panel]
    const int k8 = t & 7, rsub = t >> 3;
    const double *prow[4];
    bool vrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int grow = (j < 2 ? T.x : T.y) * ASM_TILE + ((rsub + 64 * j) & 127);
        vrow[j] = grow < p;
        prow[j] = Lb + (size_t)(vrow[j] ? grow : 0) * LDB + k8;
    }
    const double sA = cross ? d.rho : 1.0;     // row-panel scale while staging
    const int K4 = (K + 3) & ~3, nch = (K4 + MKC - 1) / MKC, total = nslots * nch;
    double rg[8];
    auto gload = [&](int s, int c) {           // chunk c of slot s: columns s*K + 16 c + [0, 16), those < K
        const size_t col = (size_t)s * K + MKC * c;
        const int kleft = K - MKC * c - k8;    // this thread's columns k8, k8 + 8 are valid if > 0, > 8
#pragma unroll
        for (int i = 0; i < 8; ++i) rg[i] = (vrow[i >> 1] && 8 * (i & 1) < kleft) ? prow[i >> 1][col + 8 * (i & 1)] : 0.0;
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k8 + 8 * (i & 1), row = (rsub + 64 * (i >> 1)) & 127;
            if (i < 4) As[buf][k][row] = sA * rg[i];
            else Bs[buf][k][row] = rg[i];
        }
    };
    d4 acc[2][4], acc2[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = acc2[u][v] = d4{0.0, 0.0, 0.0, 0.0};
    if (total > 0) {
        gload(0, 0);
        lstore(0);
    }
    __syncthreads();
    const int a0 = T.x * ASM_TILE + wa, b0 = T.y * ASM_TILE + wb;
    for (int i = 0, s = 0, c = 0, buf = 0; i < total; ++i, buf ^= 1) {
        const bool more = i + 1 < total;
        const bool last_chunk = c == nch - 1;
        const int sn = last_chunk ? s + 1 : s, cn = last_chunk ? 0 : c + 1;
        if (more) gload(sn, cn);
        const int nk4 = min(MKC, K4 - MKC * c);   // k extent of this chunk (a multiple of 4)
#pragma unroll
        for (int s4 = 0; s4 < MKC / 4; ++s4) {
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
        if (last_chunk) {   // the slot's product is complete: square it into acc2, restart the product
            if (cross) {
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) acc2[u][v][g] = fma(acc[u][v][g], acc[u][v][g], acc2[u][v][g]);
                        acc[u][v] = d4{0.0, 0.0, 0.0, 0.0};
                    }
            } else {        // same-shard pairs (coef 1) and, on a diagonal tile, this sample's omega
                int sb[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) sb[v] = shard_of[1][wb + 16 * v + r];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int ra = wa + 16 * u + q + 4 * g, a = T.x * ASM_TILE + ra;
                        const int sa = shard_of[0][ra];
                        const double dg = (diag && a < p) ? wslot[(size_t)a * B + s] : 0.0;
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int b = b0 + 16 * v + r;
                            double tv = ((sb[v] == sa) ? 1.0 : d.rho) * acc[u][v][g];
                            if (a == b) tv += dg;
                            acc2[u][v][g] = fma(tv, tv, acc2[u][v][g]);
                        }
                    }
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] = d4{0.0, 0.0, 0.0, 0.0};
            }
        }
        if (more) lstore(buf ^ 1);
        __syncthreads();
        s = sn;
        c = cn;
    }
    // epilogue: Sigma2 tile += acc2 / effsamp, the wave's (u, v, h) slices as 16-byte accesses; the
    // strict upper part of a diagonal tile and the rows past p stay zero (as in Sigma)
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

void launch_assemble_m2(const Dims &d, const Bufs &b, const double *Lb, const double *wslot, int nslots, int B,
                        double inv_eff, hipStream_t s) {
    if (b.ntiles == 0 || nslots == 0) return;
    hipLaunchKernelGGL(k_assemble_m2, dim3(b.ntiles), dim3(M2_THREADS), 0, s, d, Lb, b.LDB, nslots, wslot, B,
                       inv_eff, b.tiles, b.T0, b.Sigma2);
}

}  // namespace dcfm
