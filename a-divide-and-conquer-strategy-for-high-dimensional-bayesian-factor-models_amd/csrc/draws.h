// The variate generator of the side-stream layouts (k_draws) and the Z draw's normals.
//
// k_draws: every standard variate one iteration consumes, from
// the counter-based Philox stream, into buffers with the injected-draw layout
// (T = 1).  ALU-bound; it runs on the side stream one iteration ahead, overlapping
// the HBM-bound Y passes, so the sweep kernels only load their variates.
// Segments (wave-aligned): NZ pairs (local shards), NX pairs, NL pairs (local),
// Gpsi (local), Gps (local), Gdelta (all g shards: every rank runs every chain).
// Pointers are indexed by GLOBAL shard mg (as the injected full-g arrays are).
#pragma once
#include "dcfm_internal.h"
#include "philox.h"
#include "linalg.h"

namespace dcfm {

// Block plan of k_draws: every segment gets whole blocks, and a block covers
// 256 / LR rows of one shard with LR in {16, 32, 64} lanes per row (the smallest that
// holds a row's pairs / gammas, K <= 128), so a thread's (shard, row, index) comes
// from shifts and one block-uniform division — no per-element integer division.
// The rejection-sampled gammas (delta: one per thread; ps: one per thread) come first
// in block order so their longer threads start early; the bulk normals follow.
struct DrawPlan {
    int lrn, lrg;                    // lanes per row: normal pairs, gamma row (Gpsi)
    int nrb_n, nrb_p, nrb_g, nrb_s;  // row-blocks per shard: n rows, P rows (normals), P rows (Gpsi), Gps
    int b_gdel, b_gps, b_gpsi, b_nz, b_nx, total;  // segment end blocks (cumulative); NL last
};
__host__ __device__ inline int lanes_for(int c) { return c <= 16 ? 16 : (c <= 32 ? 32 : 64); }
__host__ __device__ inline DrawPlan draw_plan(const Dims &d) {
    DrawPlan pl;
    const int kp2 = (d.K + 1) / 2;
    pl.lrn = lanes_for(kp2);
    pl.lrg = lanes_for(d.K);
    const int rpn = 256 / pl.lrn, rpg = 256 / pl.lrg;
    pl.nrb_n = (d.n + rpn - 1) / rpn;
    pl.nrb_p = (d.P + rpn - 1) / rpn;
    pl.nrb_g = (d.P + rpg - 1) / rpg;
    pl.nrb_s = (d.P + 255) / 256;
    pl.b_gdel = (d.g * d.K + 255) / 256;          // Gdelta of all g shards
    pl.b_gps = pl.b_gdel + d.G * pl.nrb_s;
    pl.b_gpsi = pl.b_gps + d.G * pl.nrb_g;
    pl.b_nz = pl.b_gpsi + d.G * pl.nrb_n;
    pl.b_nx = pl.b_nz + pl.nrb_n;
    pl.total = pl.b_nx + d.G * pl.nrb_p;
    return pl;
}

// normals of one row: lane pair index pr = 0..kp2-1 -> out[2 pr], out[2 pr + 1]
__device__ __forceinline__ void draw_normal_row(const Rng &rng, uint32_t site, uint32_t mg, uint32_t row,
                                                uint32_t it, int K, int lane, int lr, double *out) {
    const int kp2 = (K + 1) / 2;
    for (int pr = lane; pr < kp2; pr += lr) {
        double n0, n1;
        rng.normal2(site, mg, row, (uint32_t)pr, it, n0, n1);
        out[2 * pr] = n0;
        if (2 * pr + 1 < K) out[2 * pr + 1] = n1;
    }
}

// two launches per iteration: the gamma segments (rejection loops, more registers)
// and the normal segments (high occupancy); b_off = first block of the launch
// block b of the draw plan (256 threads)
template <bool GAMMAS>
__device__ __forceinline__ void draws_block(const Dims &d, const DrawsDev &dr, int64_t iter, const DrawPlan &pl,
                                            int b) {
    const Rng rng(d.seed);
    const uint32_t it = (uint32_t)iter;
    const int t = threadIdx.x, K = d.K;
    if (GAMMAS) {
    if (b < pl.b_gdel) {                               // dc:158,163 delta, K x g, all shards
        const int x = b * 256 + t;
        if (x >= d.g * K) return;
        const int h = x % K, mg = x / K;
        const double shape = (h == 0) ? d.ad1 + 0.5 * d.P * d.K : d.ad2 + 0.5 * d.P * (d.K - h);
        const_cast<double *>(dr.Gdelta)[(size_t)mg * K + h] = rng.gamma(shape, SITE_DELTA, (uint32_t)mg, 0, (uint32_t)h, it);
        return;
    }
    if (b < pl.b_gps) {                                // dc:170 ps, P x g, shape as + n/2
        const int bb = b - pl.b_gdel, m = bb / pl.nrb_s, j = (bb % pl.nrb_s) * 256 + t;
        if (j >= d.P) return;
        const uint32_t mg = (uint32_t)(d.shard0 + m);
        const_cast<double *>(dr.Gps)[(size_t)mg * d.P + j] = rng.gamma(d.as_ + 0.5 * d.n, SITE_PS, mg, (uint32_t)j, 0, it);
        return;
    }
    if (b < pl.b_gpsi) {                               // dc:150 psi, device layout [g][P][K]
        const int bb = b - pl.b_gps, m = bb / pl.nrb_g, rb = bb % pl.nrb_g;
        const int sh = pl.lrg == 16 ? 4 : (pl.lrg == 32 ? 5 : 6);
        const int j = rb * (256 / pl.lrg) + (t >> sh), lane = t & (pl.lrg - 1);
        if (j >= d.P) return;
        const uint32_t mg = (uint32_t)(d.shard0 + m);
        double *o = const_cast<double *>(dr.Gpsi) + ((size_t)mg * d.P + j) * K;
        const double shape = d.df * 0.5 + 0.5;
        for (int k = lane; k < K; k += pl.lrg) o[k] = rng.gamma(shape, SITE_PSI, mg, (uint32_t)j, (uint32_t)k, it);
        return;
    }
    return;
    }
    const int sh = pl.lrn == 16 ? 4 : (pl.lrn == 32 ? 5 : 6), lane = t & (pl.lrn - 1), rsub = t >> sh;
    if (b < pl.b_nx) {                                 // dc:104 Z (K x n x g), dc:126 X (K x n)
        const bool xs = b >= pl.b_nz;
        const int bb = xs ? b - pl.b_nz : b - pl.b_gpsi;
        const int m = xs ? 0 : bb / pl.nrb_n, rb = xs ? bb : bb % pl.nrb_n;
        const int i = rb * (256 / pl.lrn) + rsub;
        if (i >= d.n) return;
        const uint32_t mg = xs ? 0u : (uint32_t)(d.shard0 + m);
        double *o = xs ? const_cast<double *>(dr.NX) + (size_t)i * K
                       : const_cast<double *>(dr.NZ) + ((size_t)mg * d.n + i) * K;
        draw_normal_row(rng, xs ? SITE_X : SITE_Z, mg, (uint32_t)i, it, K, lane, pl.lrn, o);
        return;
    }
    {                                                  // dc:142 Lambda (K x P x g)
        const int bb = b - pl.b_nx, m = bb / pl.nrb_p, rb = bb % pl.nrb_p;
        const int j = rb * (256 / pl.lrn) + rsub;
        if (j >= d.P) return;
        const uint32_t mg = (uint32_t)(d.shard0 + m);
        draw_normal_row(rng, SITE_LAMBDA, mg, (uint32_t)j, it, K, lane, pl.lrn,
                        const_cast<double *>(dr.NL) + ((size_t)mg * d.P + j) * K);
    }
}

// eps[i][kk], kk = 8t + 2q + e of the Z draw (dc:104 normrnd): the injected draw buffer, or
// generated here — Philox pair 4t + q of (SITE_Z, shard, row i) = normals kk, kk + 1
__device__ __forceinline__ void z_eps(const Dims &d, const DrawsDev &dr, int64_t iter, int mg, int i, bool live, int q,
                                      d2 (&ev)[4]) {
    if (d.inject) {
        const double *nz = dr.NZ + (((size_t)(iter - dr.first_iter) * d.g + mg) * d.n + (live ? i : 0)) * d.K;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int kk = 8 * t + 2 * q;
            ev[t].x = (live && kk < d.K) ? nz[kk] : 0.0;
            ev[t].y = (live && kk + 1 < d.K) ? nz[kk + 1] : 0.0;
        }
    } else {
        const Rng rng(d.seed);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int kk = 8 * t + 2 * q;
            double n0 = 0.0, n1 = 0.0;
            if (live && kk < d.K) rng.normal2(SITE_Z, (uint32_t)mg, (uint32_t)i, (uint32_t)(4 * t + q), (uint32_t)iter, n0, n1);
            ev[t].x = n0;
            ev[t].y = (kk + 1 < d.K) ? n1 : 0.0;
        }
    }
}

}  // namespace dcfm
