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
//   k_corr        k_assemble_m2's tile loop over Lb with the scale applied while staging: the row panel times
//                 s_a(s) (times rho on a cross-shard tile), the column panel times s_b(s).  Lb is only read.
// Every rank holds the gathered Lb / wslot of all shards: it computes all p scales and communalities (identical
// on every rank) and the tiles it owns.
#include "dcfm_internal.h"
#include "linalg.h"

namespace dcfm {

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

// ============================================================================
// k_corr: k_assemble_m2's tile list, XCD remap, block-sharding, wave tile (8 waves, each 32 x 64) and tile-packed
// layout, into C and C2 at once: the panels are read once per flush.  Per 128 x 128 lower tile the slots run one
// after the other; a slot's K columns of Lb are staged in chunks of 16 predicated on k < K, each value times its
// row's scale of that slot (cscale, through LDS).  After the slot's last chunk t is the
// product (times c_ab per pair on a mixed tile, 1 on the diagonal): acc1 += t, acc2 = fma(t, t, acc2), and the
// product restarts.  64 product + 64 mean + 64 square accumulator VGPRs; one read-modify-write of both tiles
// at the end of the batch, with 1 / effsamp.  The read-out writes the diagonal from the saved count
// (sigma_out.hip), so what lands on it here (nslots / effsamp per flush) is never read.
// ============================================================================
constexpr int RKC = ASM_KC, RLD = ASM_TILE + 16, CORR_THREADS = 512;

__global__ __launch_bounds__(CORR_THREADS) void k_corr(Dims d, const double *__restrict__ Lb, int LDB, int nslots,
                                                       const double *__restrict__ cscale, int B, double inv_eff,
                                                       const int2 *__restrict__ tiles, int T0,
                                                       double *__restrict__ C1, double *__restrict__ C2) {
    __shared__ double As[2][RKC][RLD], Bs[2][RKC][RLD];
    __shared__ int shard_of[2][ASM_TILE];      // shard of the tile's rows / columns
    __shared__ double Ss[3][2 * ASM_TILE];     // scales of the tile's rows | columns, slot s in Ss[s % 3]
    const int2 T = tiles[xcd_remap(blockIdx.x, gridDim.x)];
    const size_t toff = (size_t)(tri(T.x) - tri(T0) + T.y) * ASM_TILE * ASM_TILE;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (t < 2 * ASM_TILE) shard_of[t >> 7][t & 127] = ((t < ASM_TILE ? T.x : T.y) * ASM_TILE + (t & 127)) / d.P;
    const int r = lane & 15, q = lane >> 4;
    const int p = d.p, K = d.K;
    const int w4 = wave >> 1, u0 = 2 * (wave & 1);           // k_assemble's wave and first 16-row tile
    const int wa = (w4 >> 1) * 64 + 16 * u0, wb = (w4 & 1) * 64;
    const int clast = min(p, T.y * ASM_TILE + ASM_TILE) - 1;
    const bool cross = (T.x * ASM_TILE) / d.P > clast / d.P;  // as k_assemble: coef = rho everywhere
    const bool diag = T.x == T.y;
    // global -> LDS as k_assemble_m2: value i of thread t is column (t & 7) + 8 (i & 1) of row
    // (t >> 3) + 64 (i >> 1) of [row panel | column panel]
    const int k8 = t & 7, rsub = t >> 3;
    const double *prow[4];
    bool vrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int grow = (j < 2 ? T.x : T.y) * ASM_TILE + ((rsub + 64 * j) & 127);
        vrow[j] = grow < p;
        prow[j] = Lb + (size_t)(vrow[j] ? grow : 0) * LDB + k8;
    }
    const double sA = cross ? d.rho : 1.0;     // on the row panel, beside its scale
    const int K4 = (K + 3) & ~3, nch = (K4 + RKC - 1) / RKC, total = nslots * nch;
    // the scales go through LDS too (a thread's four rows' scales in registers do not fit beside three
    // accumulator sets): thread t < 256 fetches the scale of row t of [row panel | column panel], zero past p,
    // times rho on the row panel of a cross-shard tile; Ss holds three consecutive slots, slot s + 2 is written
    // while slot s's first chunk is multiplied and first read, behind a barrier, when slot s + 1 is staged
    const int srow = (t < ASM_TILE ? T.x : T.y) * ASM_TILE + (t & 127);
    auto sload = [&](int s) {
        return (t < 2 * ASM_TILE && srow < p && s < nslots) ? (t < ASM_TILE ? sA : 1.0) * cscale[(size_t)srow * B + s] : 0.0;
    };
    double rg[8], sreg = 0.0;
    auto gload = [&](int s, int c) {           // chunk c of slot s: columns s*K + 16 c + [0, 16), those < K
        const size_t col = (size_t)s * K + RKC * c;
        const int kleft = K - RKC * c - k8;    // this thread's columns k8, k8 + 8 are valid if > 0, > 8
#pragma unroll
        for (int i = 0; i < 8; ++i) rg[i] = (vrow[i >> 1] && 8 * (i & 1) < kleft) ? prow[i >> 1][col + 8 * (i & 1)] : 0.0;
    };
    auto lstore = [&](int buf, int s3) {       // s3: the chunk's slot mod 3
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k8 + 8 * (i & 1), row = (rsub + 64 * (i >> 1)) & 127;
            const double v = Ss[s3][(i < 4 ? 0 : ASM_TILE) + row] * rg[i];
            if (i < 4) As[buf][k][row] = v;
            else Bs[buf][k][row] = v;
        }
    };
    d4 acc[2][4], acc1[2][4], acc2[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = acc1[u][v] = acc2[u][v] = d4{0.0, 0.0, 0.0, 0.0};
    if (t < 2 * ASM_TILE) {
        Ss[0][t] = sload(0);
        Ss[1][t] = sload(1);
    }
    __syncthreads();
    if (total > 0) {
        gload(0, 0);
        lstore(0, 0);
    }
    __syncthreads();
    const int a0 = T.x * ASM_TILE + wa, b0 = T.y * ASM_TILE + wb;
    for (int i = 0, s = 0, s3 = 0, c = 0, buf = 0; i < total; ++i, buf ^= 1) {
        const bool more = i + 1 < total;
        const bool last_chunk = c == nch - 1;
        const int sn = last_chunk ? s + 1 : s, cn = last_chunk ? 0 : c + 1;
        const int sn3 = last_chunk ? (s3 == 2 ? 0 : s3 + 1) : s3;
        if (more) gload(sn, cn);
        if (c == 0) sreg = sload(s + 2);       // block-uniform
        const int nk4 = min(RKC, K4 - RKC * c);   // k extent of this chunk (a multiple of 4)
#pragma unroll
        for (int s4 = 0; s4 < RKC / 4; ++s4) {
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
        if (last_chunk) {   // the slot's R(s) tile is complete: into both moments, restart the product
            if (cross) {
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            acc1[u][v][g] += acc[u][v][g];
                            acc2[u][v][g] = fma(acc[u][v][g], acc[u][v][g], acc2[u][v][g]);
                        }
                        acc[u][v] = d4{0.0, 0.0, 0.0, 0.0};
                    }
            } else {        // same-shard pairs (coef 1) beside cross pairs, and the unit diagonal
                int sb[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) sb[v] = shard_of[1][wb + 16 * v + r];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int ra = wa + 16 * u + q + 4 * g, a = T.x * ASM_TILE + ra;
                        const int sa = shard_of[0][ra];
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int b = b0 + 16 * v + r;
                            double tv = ((sb[v] == sa) ? 1.0 : d.rho) * acc[u][v][g];
                            if (diag && a == b) tv = 1.0;
                            acc1[u][v][g] += tv;
                            acc2[u][v][g] = fma(tv, tv, acc2[u][v][g]);
                        }
                    }
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] = d4{0.0, 0.0, 0.0, 0.0};
            }
        }
        if (more) lstore(buf ^ 1, sn3);
        if (c == 0 && t < 2 * ASM_TILE) Ss[s3 == 0 ? 2 : s3 - 1][t] = sreg;   // slot s + 2
        __syncthreads();
        s = sn;
        s3 = sn3;
        c = cn;
    }
    // epilogue: both tiles += acc / effsamp, the wave's (u, v, h) slices as 16-byte accesses; the strict upper
    // part of a diagonal tile and the rows past p stay zero (as in Sigma)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        double *__restrict__ St = (m ? C2 : C1) + toff;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    d2 *ptr = reinterpret_cast<d2 *>(St + sig_tile_off(u0 + u, v, 2 * h, w4, lane));
                    const int b = b0 + 16 * v + r, a = a0 + 16 * u + q + 8 * h;
                    const double x = m ? acc2[u][v][2 * h] : acc1[u][v][2 * h];
                    const double y = m ? acc2[u][v][2 * h + 1] : acc1[u][v][2 * h + 1];
                    d2 o = __builtin_nontemporal_load(ptr);
                    o.x += (a < p && b <= a) ? inv_eff * x : 0.0;
                    o.y += (a + 4 < p && b <= a + 4) ? inv_eff * y : 0.0;
                    __builtin_nontemporal_store(o, ptr);
                }
    }
}

void launch_corr(const Dims &d, const Bufs &b, const Corr &cr, const double *Lb, const double *wslot, int nslots,
                 int B, double inv_eff, hipStream_t s) {
    if (nslots == 0) return;
    const int per = 256 / CS_LANES;
    hipLaunchKernelGGL(k_corr_scale, dim3((d.p + per - 1) / per), dim3(256), 0, s, Lb, b.LDB, wslot, B, d.p, d.K,
                       nslots, inv_eff, cr.cscale, cr.H, cr.H2);
    if (b.ntiles == 0) return;
    hipLaunchKernelGGL(k_corr, dim3(b.ntiles), dim3(CORR_THREADS), 0, s, d, Lb, b.LDB, nslots, cr.cscale, B, inv_eff,
                       b.tiles, b.T0, cr.C, cr.C2);
}

}  // namespace dcfm
