// Covariance assembly (divideconquer.m:180-195): the saved samples of a batch (k_save), their
// accumulation into this rank's tile-packed block of Sigmaout on the assembly stream (k_assemble),
// and the packed column stripes of the output gather (k_sigma_pack / k_sigma_unpack).
#include "dcfm_internal.h"
#include "linalg.h"

#include <algorithm>

namespace dcfm {

// ============================================================================
// saved samples: Lb[(mg*P + j)][slot*K + k] = Lambda, wsum += omega         dc:180-186
// M2 (DCFM_FLAG_SIGMA_M2): also the sample's own omega, wslot[(mg*P + j)][slot] of B slots
// K > 32, and K <= 32 with DCFM_FLAG_EXACT_RESIDUAL (omega rewritten after k_lambda); otherwise k_lambda
// writes the same values itself (SaveArgs, lambda.h) and this launch does not run
// ============================================================================
template <bool M2>
__global__ __launch_bounds__(256) void k_save(Dims d, const double *__restrict__ Lam,
                                              const double *__restrict__ omega,
                                              double *__restrict__ Lb, double *__restrict__ wsum,
                                              int LDB, int slot, double *__restrict__ wslot, int B) {
    const size_t total = (size_t)d.G * d.P * d.K;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total;
         e += (size_t)gridDim.x * blockDim.x) {
        const int k = e % d.K;
        const size_t jm = e / d.K;
        const int j = jm % d.P, m = jm / d.P;
        const size_t a = (size_t)(d.shard0 + m) * d.P + j;
        Lb[a * LDB + (size_t)slot * d.K + k] = Lam[((size_t)m * d.PP + j) * d.kp + k];
        if (k == 0) {
            const double w = omega[(size_t)m * d.PP + j];
            wsum[a] += w;
            if (M2) wslot[a * B + slot] = w;
        }
    }
}

// ============================================================================
// k_assemble: Sigma[a][b] += (coef(a,b)/effsamp) sum_kk Lb[a][kk] Lb[b][kk]
//                            + [a==b] wsum[a]/effsamp                       dc:184-195
// coef = 1 inside a diagonal shard block (Lambda_r Lambda_r' + Omega_r), rho
// across blocks (rho Lambda_r Lambda_c').  Lower-triangle 128x128 tiles only, in
// 8 x 8-tile supertiles (dcfm_create), XCD-contiguous (xcd_remap): the tiles an XCD
// has in flight share 8 row and 8 column panels of Lb in its L2.  The tile's place
// in the rank's packed Sigma block comes from (ti, tj).
// Cross-shard tiles (no row and column of the same shard: coef = rho everywhere, ~95% of
// the tiles at c3) start their accumulators FROM the old Sigma values, loaded with the
// first panel chunk, and stage the row panel scaled by rho / effsamp: the epilogue is
// plain stores, so the read half of the read-modify-write never waits at the end of the
// tile.  Tiles with same-shard pairs (and the diagonal) keep the epilogue update.  Sigma is
// streamed with nontemporal loads / stores (read and written once per flush): it no longer
// evicts the Lb panels the XCD's co-resident tiles share from L2 (driver flush 1,176 -> 1,137 us;
// a second register set prefetching the panels two chunks ahead measured no gain).
// 4 waves in 2x2, each 64x64 = 4x4 tiles of v_mfma_f64_16x16x4.  The k extent
// (batch x K) runs in chunks of 16 through double-buffered LDS, stored k-major
// with a 144-double pitch: an MFMA operand read (16 consecutive rows x 4 k) is a
// conflict-free ds_read_b64, and the next chunk's global loads are in flight
// during the current chunk's 64 MFMAs per wave.  One barrier per chunk, in front of the
// chunk's last k-step: the operand reads run one k-step ahead of the MFMAs across the
// chunks, the next chunk is staged in the middle of the MFMA stream, and the panel loads
// carry no exec-mask branch into it (r08: driver flush 1,084 -> 942 us, 96-sample flush
// 18.80 -> 17.05 ms, Sigma bitwise unchanged).
// ============================================================================
constexpr int AKC = ASM_KC, ALD = ASM_TILE + 16, ASM_THREADS = 256;
// A/B switches of the chunk loop (tools/build_variant.sh; profiles/r06_ab_summary.txt, r08)
#ifndef DCFM_ASM_PIPE
#define DCFM_ASM_PIPE 1        // 0: the A/B baseline, one loop with a break for the partial last chunk
#endif
#ifndef DCFM_ASM_GLB
#define DCFM_ASM_GLB 1         // 0: the A/B baseline, the panel loads of rows past p predicated (a branch per load)
#endif
constexpr bool ASM_GLB = DCFM_ASM_GLB;
#ifndef DCFM_ASM_LSTORE_AT
#define DCFM_ASM_LSTORE_AT 2   // the next chunk's LDS stores follow this k-step of the chunk (1 .. 3)
#endif

__device__ __forceinline__ void assemble_tile(const Dims &d, const double *__restrict__ Lb, int LDB, int kext,
                                              const double *__restrict__ wsum, double inv_eff, int2 T, int T0,
                                              double *__restrict__ Sig, double (*As)[AKC][ALD],
                                              double (*Bs)[AKC][ALD], int (*shard_of)[ASM_TILE]) {
    double *__restrict__ St = Sig + (size_t)(tri(T.x) - tri(T0) + T.y) * ASM_TILE * ASM_TILE;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    shard_of[t >> 7][t & 127] = ((t < ASM_TILE ? T.x : T.y) * ASM_TILE + (t & 127)) / d.P;
    const int r = lane & 15, q = lane >> 4;
    const int p = d.p;
    const int wa = (wave >> 1) * 64, wb = (wave & 1) * 64;
    // cross-shard tile: the rows' shards all lie below the columns' (tj < ti, rows >= columns)
    const int clast = min(p, T.y * ASM_TILE + ASM_TILE) - 1;
    const bool cross = (T.x * ASM_TILE) / d.P > clast / d.P;
    const double sA = cross ? d.rho * inv_eff : 1.0;     // row-panel scale while staging
    // global -> LDS: thread t stages row (t >> 1) of both panels, k = 8 (t & 1) .. +7
    const int srow = t >> 1, shalf = t & 1;
    const int ga = T.x * ASM_TILE + srow, gb = T.y * ASM_TILE + srow;
    const bool va = ga < p, vb = gb < p;
    const double *pa = Lb + (size_t)(va ? ga : 0) * LDB + 8 * shalf;
    const double *pb = Lb + (size_t)(vb ? gb : 0) * LDB + 8 * shalf;
    const d2 zero2 = {0.0, 0.0};
    d2 ra[4], rb[4];
    // rows past p: the loads go to row 0 (pa, pb) without a branch and the staging writes zeros (a load under
    // `va ? ... : 0` compiles to an exec-mask branch per load: eight in every chunk's MFMA stream)
    auto gload = [&](int kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (ASM_GLB) {
                ra[i] = *reinterpret_cast<const d2 *>(pa + kc + 2 * i);
                rb[i] = *reinterpret_cast<const d2 *>(pb + kc + 2 * i);
            } else {
                ra[i] = va ? *reinterpret_cast<const d2 *>(pa + kc + 2 * i) : zero2;
                rb[i] = vb ? *reinterpret_cast<const d2 *>(pb + kc + 2 * i) : zero2;
            }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 8 * shalf + 2 * i;
            As[buf][k][srow] = ASM_GLB && !va ? 0.0 : sA * ra[i].x;
            As[buf][k + 1][srow] = ASM_GLB && !va ? 0.0 : sA * ra[i].y;
            Bs[buf][k][srow] = ASM_GLB && !vb ? 0.0 : rb[i].x;
            Bs[buf][k + 1][srow] = ASM_GLB && !vb ? 0.0 : rb[i].y;
        }
    };
    gload(0);      // ahead of the tile's Sigma loads: staging chunk 0 waits only for its panels
    d4 acc[4][4];
    // the tile's values of this wave's accumulators: slice (u, v, h) = 64 lanes x 16 B, contiguous
    auto sl = [&](int u, int v, int h) { return reinterpret_cast<d2 *>(St + sig_tile_off(u, v, 2 * h, wave, lane)); };
    if (cross) {   // acc = the tile's old values (C/D layout: row q + 4g of 16-row tile u)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const d2 o = __builtin_nontemporal_load(sl(u, v, h));
                    acc[u][v][2 * h] = o.x;
                    acc[u][v][2 * h + 1] = o.y;
                }
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = d4{0.0, 0.0, 0.0, 0.0};
    }
    lstore(0);
    __syncthreads();
    // one k-step: the wave's operands of k = 4 s4 .. + 3 from LDS, and its 16 MFMAs
    auto opload = [&](int buf, int s4, double (&a)[4], double (&b)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = As[buf][4 * s4 + q][wa + 16 * u + r];
#pragma unroll
        for (int v = 0; v < 4; ++v) b[v] = Bs[buf][4 * s4 + q][wb + 16 * v + r];
    };
    auto mma = [&](const double (&a)[4], const double (&b)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = mfma16x16x4(a[u], b[v], acc[u][v]);
    };
#if DCFM_ASM_PIPE
    // Whole chunks run in a loop of NS k-steps without a branch between them; the last chunk (1 .. NS
    // k-steps) follows it.  The operand reads run one k-step ahead of the MFMAs, across the chunks: a
    // chunk's barrier stands in front of its LAST k-step's MFMAs, whose operands are in registers by then,
    // and the next chunk's first operands are read right behind it, under those 16 MFMAs.  The next chunk's
    // panels (loaded at the chunk's head) are staged after k-step LAT, one k-step ahead of the barrier, so
    // their LDS stores are not what the barrier's arrival waits for.  Every accumulator takes the same
    // products in the same k order as the plain loop.
    constexpr int NS = AKC / 4, LAT = DCFM_ASM_LSTORE_AT;
    static_assert(1 <= LAT && LAT < NS, "the staging precedes the chunk's barrier");
    const int nch = (kext + AKC - 1) / AKC;             // chunks; all but the last are whole
    const int nlast = (kext - (nch - 1) * AKC) / 4;     // k-steps of the last one, 1 .. NS (kext is a multiple of 4)
    double a[2][4], b[2][4];
    int buf = 0;
    opload(0, 0, a[0], b[0]);
    for (int c = 0; c < nch - 1; ++c, buf ^= 1) {
        gload((c + 1) * AKC);
#pragma unroll
        for (int s4 = 0; s4 < NS; ++s4) {
            if (s4 + 1 < NS) {
                opload(buf, s4 + 1, a[(s4 + 1) & 1], b[(s4 + 1) & 1]);
            } else {
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
                opload(buf ^ 1, 0, a[0], b[0]);
                __builtin_amdgcn_sched_barrier(0);
            }
            mma(a[s4 & 1], b[s4 & 1]);
            if (s4 + 1 == LAT) {
                // the wait for the panels belongs HERE: neither the scheduler nor the optimiser may lift the
                // staging's row scaling, and with it the wait, to the head of the chunk
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(ra[i]), "+v"(rb[i]));
                lstore(buf ^ 1);
            }
        }
    }
    // the last chunk (block-uniform count); its first operands are in a[0], b[0]
    mma(a[0], b[0]);
#pragma unroll
    for (int s4 = 1; s4 < NS; ++s4) {
        if (s4 >= nlast) break;
        opload(buf, s4, a[1], b[1]);
        mma(a[1], b[1]);
    }
#else
    for (int kc = 0, buf = 0; kc < kext; kc += AKC, buf ^= 1) {
        const bool more = kc + AKC < kext;
        if (more) gload(kc + AKC);
        const int nk4 = min(AKC, kext - kc);   // k extent of this chunk (a multiple of 4)
#pragma unroll
        for (int s4 = 0; s4 < AKC / 4; ++s4) {
            if (4 * s4 >= nk4) break;            // block-uniform: the last chunk may be partial
            double a[4], b[4];
            opload(buf, s4, a, b);
            mma(a, b);
        }
        if (more) lstore(buf ^ 1);
        __syncthreads();
    }
#endif
    if (cross) {   // acc = old + (rho / effsamp) L_a L_b': plain stores (the whole tile is below the diagonal)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    d2 o;
                    o.x = acc[u][v][2 * h];
                    o.y = acc[u][v][2 * h + 1];
                    __builtin_nontemporal_store(o, sl(u, v, h));
                }
        return;
    }
    // epilogue: lower-triangle read-modify-write of the tile (tile-packed, accumulator order inside),
    // loads issued together (predicated, no branches around them), shard test from the LDS table
    const int a0 = T.x * ASM_TILE + wa, b0 = T.y * ASM_TILE + wb;
    int sb[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) sb[v] = shard_of[1][wb + 16 * v + r];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        double old[4][4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int a = a0 + 16 * u + q + 4 * g;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int b = b0 + 16 * v + r;
                const bool live = a < p && b <= a;
                old[g][v] = live ? __builtin_nontemporal_load(&St[sig_tile_off(u, v, g, wave, lane)]) : 0.0;
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int a = a0 + 16 * u + q + 4 * g;
            const int sa = shard_of[0][wa + 16 * u + q + 4 * g];
            const double dg = (a < p) ? wsum[a] * inv_eff : 0.0;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int b = b0 + 16 * v + r;
                if (a < p && b <= a) {
                    const double coef = (sb[v] == sa) ? 1.0 : d.rho;
                    double val = coef * acc[u][v][g] * inv_eff;
                    if (a == b) val += dg;
                    __builtin_nontemporal_store(old[g][v] + val, &St[sig_tile_off(u, v, g, wave, lane)]);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256, 2) void k_assemble(Dims d, const double *__restrict__ Lb, int LDB,
                                                     int kext, const double *__restrict__ wsum,
                                                     double inv_eff, const int2 *__restrict__ tiles, int T0,
                                                     double *__restrict__ Sig) {
    __shared__ double As[2][AKC][ALD], Bs[2][AKC][ALD];
    __shared__ int shard_of[2][ASM_TILE];      // shard of the tile's rows / columns (epilogue coef)
    assemble_tile(d, Lb, LDB, kext, wsum, inv_eff, tiles[xcd_remap(blockIdx.x, gridDim.x)], T0, Sig, As, Bs,
                  shard_of);
}

// Column stripe [c0, c0 + nc) of the symmetric Sigmaout from this rank's tile-packed block
// of the lower triangle (tile rows [T0, T1), rows [R0, R1)), written as the rank's packed
// windows: column c holds rows [win_lo(c), R1) at out + win_off(c) (dc:194-195 output, Q9:
// the symmetrisation is this mirror).  One rank owns everything: the windows are then the
// dense p x nc column-major stripe.  32x32 tiles: Sigma(r, c) = S(r, c) for r >= c (read
// along c, transposed through LDS), S(c, r) for r < c (read along r).
// WHICH (DCFM_SIGMA_*): the mean S, the second moment S2, or the posterior standard deviation
// sqrt(max(0, rs S2 - (rs S)^2)) formed here from both (rs = effsamp / saved samples), so
// neither matrix leaves the device to be combined.
// dset: the diagonal is not read but set to dval (the partial correlations: R(s)_aa = 1 for every sample, so
// both moments are saved / effsamp and the standard deviation 0 by definition, not by a rounded sum)
template <int WHICH>
__global__ __launch_bounds__(256) void k_sigma_pack(const double *__restrict__ S, const double *__restrict__ S2,
                                                    double rs, int p, int T0, int T1, int c0, int nc,
                                                    double *__restrict__ out, int dset, double dval) {
    auto at = [&](size_t o) {
        if (WHICH == 0) return S[o];
        if (WHICH == 1) return S2[o];
        const double m = rs * S[o];
        return sqrt(fmax(0.0, fma(rs, S2[o], -m * m)));
    };
    __shared__ double lo[32][33];
    const int R0 = min(p, T0 * ASM_TILE), R1 = min(p, T1 * ASM_TILE);
    const int r0 = blockIdx.x * 32, cb = c0 + blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const bool need_lo = r0 + 31 >= cb;            // some r >= c in the tile
    const bool need_up = r0 < cb + 31;             // some r < c
    if (need_lo) {
        for (int yy = ty; yy < 32; yy += 8) {      // rows r = r0 + yy, columns c = cb + tx
            const int r = r0 + yy, c = cb + tx;
            lo[yy][tx] = (r >= R0 && r < R1 && c < c0 + nc && r >= c) ? ((dset && r == c) ? dval : at(sig_off(r, c, T0))) : 0.0;
        }
    }
    __syncthreads();
    for (int yy = ty; yy < 32; yy += 8) {          // output column c = cb + yy, rows r = r0 + tx
        const int c = cb + yy, r = r0 + tx;
        if (c >= c0 + nc || r >= R1) continue;
        const long long wl = win_lo(c, R0, R1);
        if (r < wl) continue;
        const double v = (r >= c) ? lo[tx][yy] : (need_up ? at(sig_off(c, r, T0)) : 0.0);
        out[win_off(c, c0, R0, R1) + (r - wl)] = v;
    }
}

// Root of the striped gather: out (dense p x nc, column-major) from the ranks' packed
// windows.  Element (r, c) lives on the owner of tile row max(r, c) / 128.
__global__ __launch_bounds__(256) void k_sigma_unpack(const double *__restrict__ recv, int p, int c0, int cbeg,
                                                      const int *__restrict__ Tb,
                                                      const long long *__restrict__ base, int nranks,
                                                      double *__restrict__ out) {
    const int c = cbeg + blockIdx.y;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < p; r += gridDim.x * 256) {
        const int t = max(r, c) / ASM_TILE;
        int k = 0;
        while (k + 1 < nranks && Tb[k + 1] <= t) ++k;
        const long long R0 = min(p, Tb[k] * ASM_TILE), R1 = min(p, Tb[k + 1] * ASM_TILE);
        out[(size_t)(c - c0) * p + r] = recv[base[k] + win_off(c, c0, R0, R1) + (r - win_lo(c, R0, R1))];
    }
}

// ============================================================================
// launchers
// ============================================================================
void launch_save(const Dims &d, const Bufs &b, double *Lb, double *wsum, int slot, hipStream_t s, double *wslot,
                 int B) {
    const size_t total = (size_t)d.G * d.P * d.K;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 4096);
    if (wslot)
        hipLaunchKernelGGL(k_save<true>, dim3(grid), dim3(256), 0, s, d, b.Lam, b.omega, Lb, wsum, b.LDB, slot, wslot, B);
    else
        hipLaunchKernelGGL(k_save<false>, dim3(grid), dim3(256), 0, s, d, b.Lam, b.omega, Lb, wsum, b.LDB, slot, wslot, B);
}
void launch_assemble(const Dims &d, const Bufs &b, const double *Lb, const double *wsum, int kext,
                     double inv_eff, hipStream_t s) {
    if (b.ntiles == 0) return;
    hipLaunchKernelGGL(k_assemble, dim3(b.ntiles), dim3(ASM_THREADS), 0, s, d, Lb, b.LDB, kext, wsum, inv_eff,
                       b.tiles, b.T0, b.Sigma);
}
void launch_sigma_pack(const double *S, const double *S2, int which, double rs, int p, int T0, int T1, int c0,
                       int nc, double *out, hipStream_t s, const double *diag) {
    const int R1 = std::min(p, T1 * ASM_TILE);
    if (nc <= 0 || R1 <= 0 || T1 <= T0) return;
    const dim3 grid(cdiv(R1, 32), cdiv(nc, 32));
    const int dset = diag ? 1 : 0;
    const double dval = diag ? *diag : 0.0;
    if (which == 0)
        hipLaunchKernelGGL(k_sigma_pack<0>, grid, dim3(256), 0, s, S, S2, rs, p, T0, T1, c0, nc, out, dset, dval);
    else if (which == 1)
        hipLaunchKernelGGL(k_sigma_pack<1>, grid, dim3(256), 0, s, S, S2, rs, p, T0, T1, c0, nc, out, dset, dval);
    else hipLaunchKernelGGL(k_sigma_pack<2>, grid, dim3(256), 0, s, S, S2, rs, p, T0, T1, c0, nc, out, dset, dval);
}
void launch_sigma_unpack(const double *recv, int p, int c0, int nc, const int *Tb, const long long *base,
                         int nranks, double *out, hipStream_t s) {
    for (int j = 0; j < nc; j += 32768) {   // grid.y <= 32768 columns per launch
        const int w = std::min(32768, nc - j);
        hipLaunchKernelGGL(k_sigma_unpack, dim3(std::min(cdiv(p, 256), 16), w), dim3(256), 0, s, recv, p, c0, c0 + j,
                           Tb, base, nranks, out);
    }
}

}  // namespace dcfm
