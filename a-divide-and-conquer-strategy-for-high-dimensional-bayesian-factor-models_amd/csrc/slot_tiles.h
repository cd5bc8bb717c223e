// The per-slot tile loop of the second-moment assembly kernels (k_assemble_m2, k_assemble_pc_m2, k_corr).
// They share k_assemble's tile list, XCD remap, block-sharding and tile-packed layout (sig_tile_off), but
// k_assemble runs all samples of a batch along one k extent, so the per-sample product never exists.  Here, per
// 128 x 128 lower-triangle tile, the samples (slots) of the batch run one after the other: a slot's K columns of
// the row and column panels go through LDS in chunks of KC = 16, zero-padded to the MFMA k-step.  A slot starts
// at column s K (8-byte aligned only) and ends inside a k-step unless 4 | K, so a chunk is staged with 8-byte
// loads predicated on k < K and never touches the neighbour slot's columns.  A slot may run several phases of
// such chunks into the same product (k_assemble_pc_m2).  After the slot's last chunk the kernel's fold takes
// the product t (fma(t, t, acc2), ...) and the product accumulators restart from zero.  One read-modify-write
// of the output tile at the end of the batch (add_tile).
// 8 waves, each 32 x 64 = 2 x 4 tiles of v_mfma_f64_16x16x4: 64 accumulator VGPRs for the product and 64 per
// moment (a 64 x 64 wave tile would need 128 + 128 before operands: one wave per SIMD).  Wave w covers rows
// 32 (w & 1) .. + 31 of k_assemble's wave w >> 1, so the output tile has the layout of the Sigma tile.
// global -> LDS: a chunk is 16 columns of the 256 rows of both panels, 8 values per thread.  Lanes 8 j .. 8 j + 7
// read 8 consecutive columns of one row, so a wave's load touches 8 rows (8 to 16 cache lines; one row per lane
// pair touched 64 and left the staging bound by the L1's line rate): value i of thread t is column
// (t & 7) + 8 (i & 1) of row (t >> 3) + 64 (i >> 1) of [row panel | column panel].
#pragma once
#include "dcfm_internal.h"
#include "linalg.h"

namespace dcfm {
namespace slot {

constexpr int KC = ASM_KC, LD = ASM_TILE + 16, THREADS = 512;
typedef double Panel[2][KC][LD];   // a double-buffered chunk of one panel, [k][row]

__device__ __forceinline__ void zero(d4 (&acc)[2][4]) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = d4{0.0, 0.0, 0.0, 0.0};
}

// the block's tile and the thread's place in it: MFMA lane (r, q), k_assemble's wave w4 and first 16-row tile
// u0, the wave tile's corner in the tile (wa, wb) and in the matrix (a0, b0)
struct Tile {
    int2 T;
    size_t off;         // of the tile in the rank's tile-packed output
    int t, lane, r, q, w4, u0, wa, wb, clast;
    bool cross, diag;   // cross: every row's shard is past every column's (as k_assemble: coef = rho everywhere)
    // shard_of, if given: the shards of the tile's rows / columns, read behind the loop's first barrier.  It is
    // filled HERE, before the divisions of `cross`, and not by a helper of its own behind the constructor: k_corr
    // sits at 256 VGPRs and with the fill after `cross` it spills some 220 of them (check with make asm-corr)
    __device__ __forceinline__ Tile(const Dims &d, const int2 *__restrict__ tiles, int T0,
                                    int (*shard_of)[ASM_TILE] = nullptr) {
        T = tiles[xcd_remap(blockIdx.x, gridDim.x)];
        off = (size_t)(tri(T.x) - tri(T0) + T.y) * ASM_TILE * ASM_TILE;
        t = threadIdx.x, lane = t & 63, r = lane & 15, q = lane >> 4;
        if (shard_of && t < 2 * ASM_TILE)
            shard_of[t >> 7][t & 127] = ((t < ASM_TILE ? T.x : T.y) * ASM_TILE + (t & 127)) / d.P;
        w4 = t >> 7, u0 = 2 * ((t >> 6) & 1);
        wa = (w4 >> 1) * 64 + 16 * u0, wb = (w4 & 1) * 64;
        clast = min(d.p, T.y * ASM_TILE + ASM_TILE) - 1;
        cross = (T.x * ASM_TILE) / d.P > clast / d.P;
        diag = T.x == T.y;
    }
    __device__ __forceinline__ int a0() const { return T.x * ASM_TILE + wa; }
    __device__ __forceinline__ int b0() const { return T.y * ASM_TILE + wb; }
};

// the thread's four staged rows j (two of each panel): global row (0 past p), validity and shard; value i of a
// chunk is row i >> 1 of these, LDS element [k(i)][row(i)]
struct Rows {
    int k8, rsub, grow[4], shard[4];
    bool valid[4];
    __device__ __forceinline__ Rows(const Tile &g, const Dims &d) {
        k8 = g.t & 7, rsub = g.t >> 3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = (j < 2 ? g.T.x : g.T.y) * ASM_TILE + ((rsub + 64 * j) & 127);
            valid[j] = a < d.p, shard[j] = a / d.P, grow[j] = valid[j] ? a : 0;
        }
    }
    __device__ __forceinline__ int k(int i) const { return k8 + 8 * (i & 1); }
    __device__ __forceinline__ int row(int i) const { return (rsub + 64 * (i >> 1)) & 127; }
    // chunk c of a K-column slot holds value i
    __device__ __forceinline__ bool has(int i, int c, int K) const { return valid[i >> 1] && k(i) < K - KC * c; }
    // prow[j]: the thread's column k8 of staged row j in the row panel A (j < 2) or the column panel B, pitch ld
    __device__ __forceinline__ void pointers(const double *(&prow)[4], const double *A, const double *B, size_t ld) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) prow[j] = (j < 2 ? A : B) + grow[j] * ld + k8;
    }
    // rg: the thread's 8 values of chunk c of the K columns that start at col; zero where the chunk has none
    __device__ __forceinline__ void load(double (&rg)[8], const double *const (&prow)[4], size_t col, int c, int K) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) rg[i] = has(i, c, K) ? prow[i >> 1][col + 8 * (i & 1)] : 0.0;
    }
};

// f(u, v, e) over the thread's 32 accumulator elements
template <class F>
__device__ __forceinline__ void each(F f) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) f(u, v, e);
}

// a tile that is not cross: f(u, v, e, a, a == b, c_ab * acc[u][v][e]) over the thread's elements, row by row;
// (a, b) the element's global row and column, c_ab = 1 inside a shard and rho across
template <class F>
__device__ __forceinline__ void pairs(const Tile &g, const int (*shard_of)[ASM_TILE], double rho, const d4 (&acc)[2][4],
                                      F f) {
    int sb[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) sb[v] = shard_of[1][g.wb + 16 * v + g.r];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ra = g.wa + 16 * u + g.q + 4 * e, a = g.T.x * ASM_TILE + ra, sa = shard_of[0][ra];
#pragma unroll
            for (int v = 0; v < 4; ++v)
                f(u, v, e, a, a == g.b0() + 16 * v + g.r, ((sb[v] == sa) ? 1.0 : rho) * acc[u][v][e]);
        }
}

// The loop over nslots x nph x nch chunks, double-buffered with one barrier per chunk.  The kernel's callables:
//   gload(s, ph, c)     chunk c of phase ph of slot s, global -> the kernel's registers;
//   lstore(buf, s)      those registers (of slot s) -> As[buf], Bs[buf];
//   head(s, ph, c)      after the next chunk's loads are issued, before this chunk is multiplied;
//   tail(s, ph, c)      after the staging stores, before the barrier;
//   fold(s, acc)        the slot's product is complete; acc restarts from zero behind it.
// NPH: the phases of a slot where the kernel knows them (the odometer then carries none), 0: nph_rt of them.
template <int NPH, class GL, class LS, class HD, class TL, class FD>
__device__ __forceinline__ void loop(const Tile &g, Panel &As, Panel &Bs, int K, int nslots, int nph_rt, GL gload,
                                     LS lstore, HD head, TL tail, FD fold) {
    const int nph = NPH ? NPH : nph_rt;
    const int K4 = (K + 3) & ~3, nch = (K4 + KC - 1) / KC, total = nslots * nph * nch;
    d4 acc[2][4];
    zero(acc);
    if (total > 0) {
        gload(0, 0, 0);
        lstore(0, 0);
    }
    __syncthreads();
    for (int i = 0, s = 0, ph = 0, c = 0, buf = 0; i < total; ++i, buf ^= 1) {
        const bool more = i + 1 < total, last_chunk = c == nch - 1, last = last_chunk && (NPH == 1 || ph == nph - 1);
        const int cn = last_chunk ? 0 : c + 1, sn = last ? s + 1 : s;
        const int phn = NPH == 1 ? 0 : (last_chunk ? (last ? 0 : ph + 1) : ph);
        if (more) gload(sn, phn, cn);
        head(s, ph, c);
        const int nk4 = min(KC, K4 - KC * c);   // k extent of this chunk (a multiple of 4)
#pragma unroll
        for (int s4 = 0; s4 < KC / 4; ++s4) {
            if (4 * s4 >= nk4) break;            // block-uniform
            double a[2], b[4];
#pragma unroll
            for (int u = 0; u < 2; ++u) a[u] = As[buf][4 * s4 + g.q][g.wa + 16 * u + g.r];
#pragma unroll
            for (int v = 0; v < 4; ++v) b[v] = Bs[buf][4 * s4 + g.q][g.wb + 16 * v + g.r];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = mfma16x16x4(a[u], b[v], acc[u][v]);
        }
        if (last) {
            fold(s, acc);
            zero(acc);
        }
        if (more) lstore(buf ^ 1, sn);
        tail(s, ph, c);
        __syncthreads();
        s = sn, ph = phn, c = cn;
    }
}

// epilogue: tile St += inv_eff * acc, the wave's (u, v, h) slices as 16-byte accesses; the strict upper part of a
// diagonal tile and the rows past p stay zero (as in Sigma)
__device__ __forceinline__ void add_tile(const Tile &g, double *__restrict__ St, int p, double inv_eff,
                                         const d4 (&acc)[2][4]) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                d2 *ptr = reinterpret_cast<d2 *>(St + sig_tile_off(g.u0 + u, v, 2 * h, g.w4, g.lane));
                const int b = g.b0() + 16 * v + g.r, a = g.a0() + 16 * u + g.q + 8 * h;
                d2 o = __builtin_nontemporal_load(ptr);
                o.x += (a < p && b <= a) ? inv_eff * acc[u][v][2 * h] : 0.0;
                o.y += (a + 4 < p && b <= a + 4) ? inv_eff * acc[u][v][2 * h + 1] : 0.0;
                __builtin_nontemporal_store(o, ptr);
            }
}

}  // namespace slot
}  // namespace dcfm
