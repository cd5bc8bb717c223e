// The delta / tau stage of the sweep (divideconquer.m:154-165, 174-177): the column sums of
// psi o Lambda^2 (dc:156) and the multiplicative-gamma-process chain, one definition for every
// factor width (narrow k_delta and k_cpass<32>'s extra blocks: KW = 32; wide::k_delta: KW = 64, 128).
//   K >= 2: every shard's h>=2 step reads shard 1's ALREADY-updated delta_h (Q4);
//           each wave re-runs shard 1's chain first (deterministic, identical).
//   K == 1: cumprod over the K x 1 x g array runs along shards (Q5):
//           tau_used(m) = prod_{m'<m} delta_new(m') * delta_old(m).
// The chain over h is scalar: with T_h = sum_{l>=h} tau_l s_l of the incoming
// tau, the reference's recomputed cumprod gives dot_h = F_h T_h where
// F_h = prod_{h'<h} delta_new(h')/delta_old(h')  (exact; rounding-level only).
//   P == 1 (Q14): mat of dc:156 is 1 x K, so MATLAB's sum(mat(:,h:end)) runs along the row and
//           returns the scalar sum_{l>=h} s_l; dc:157 / dc:161 then use
//           (sum_{l>=h} tau_l)(sum_{l>=h} s_l).  The recomputed cumprod scales every tau_l, l >= h,
//           by the same F_h, so T_h = (suffix sum of the incoming tau)_h (suffix sum of s)_h and
//           the chain is the same.  K == 1 is unaffected (one term).
// Every rank runs every shard's chain (delta / tau are replicated); Plam = psi o tau' (dc:175-177)
// is formed where it is read, in the next loading-row kernel.
#pragma once
#include "dcfm_internal.h"
#include "philox.h"
#include "linalg.h"

namespace dcfm {

// ============================================================================
// column sums: sloc[m][k] = sum_{j<P} cpart[m][j][k], fixed order            dc:156 sum(mat)
// block = (shard m, 32 columns); 8 row groups x 4 independent accumulators each.
// ============================================================================
template <int KW>
__device__ __forceinline__ void colsum_tile(const Dims &d, const double *__restrict__ cpart,
                                            double *__restrict__ sloc, int m, int kt, double *smem) {
    double (*part)[32] = reinterpret_cast<double (*)[32]>(smem);
    const int k = 32 * kt + (threadIdx.x & 31), grp = threadIdx.x >> 5;
    const double *cp = cpart + (size_t)m * d.PP * KW + k;
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    // rows j = grp + 8 i: every load of a 320-row band in flight at once (one latency round
    // per band instead of one per few rows), summed into 4 accumulators in row order
    constexpr int RB = 40;
    for (int j0 = 0; j0 < d.P; j0 += 8 * RB) {
        double v[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int j = j0 + grp + 8 * i;
            v[i] = j < d.P ? cp[(size_t)j * KW] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) s4[i & 3] += v[i];
    }
    part[grp][threadIdx.x & 31] = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    __syncthreads();
    if (threadIdx.x < 32) {
        double tt = 0.0;
#pragma unroll
        for (int g2 = 0; g2 < 8; ++g2) tt += part[g2][threadIdx.x];
        sloc[(size_t)m * KW + k] = tt;
    }
}

// standard gamma of the delta site, h = 0-based factor index (dc:158,163): the injected
// buffer, or — generated draws — the counter-addressed Philox variate itself (the value
// k_draws writes), so the delta chain never depends on which draw-batch slot holds its
// iteration (the fused chain runs iteration t's chain during iteration t+1)
__device__ inline double delta_G(const Dims &d, const DrawsDev &dr, int64_t iter, int mg, int h) {
    if (d.inject) return dr.Gdelta[((size_t)(iter - dr.first_iter) * d.g + mg) * d.K + h];
    const double shape = (h == 0) ? d.ad1 + 0.5 * d.P * d.K : d.ad2 + 0.5 * d.P * (d.K - h);
    return Rng(d.seed).gamma(shape, SITE_DELTA, (uint32_t)mg, 0, (uint32_t)h, (uint32_t)iter);
}

// the chain k_cpass's extra blocks run beside the pass (fused K <= 32 layouts)
struct DeltaArgs {
    const double *delta_in, *tau_in;
    double *delta_out, *tau_out;
    int64_t iter;                          // iteration whose delta / tau the chain updates
};

// column sums of global shard mg (row stride kw) in the gathered buffer; the rank blocks are
// padded by d.sgap in the packed message of the fused several-rank layout (K <= 32), else 0
__device__ __forceinline__ size_t sall_off(const Dims &d, int mg, int kw) {
    return (size_t)mg * kw + (d.sgap ? (size_t)(mg / d.G) * d.sgap : 0);
}

// NV indices per lane, index l + 64 s in v[s]: suffix sum / inclusive product over all of them
template <int NV>
__device__ __forceinline__ void suffix_sum_nv(double (&v)[NV], int l) {
    v[NV - 1] = wave_suffix_sum(v[NV - 1], l);
    if (NV == 2) v[0] = wave_suffix_sum(v[0], l) + readlane_d(v[NV - 1], 0);
}
template <int NV>
__device__ __forceinline__ void scan_prod_nv(double (&v)[NV], int l) {
    v[0] = wave_scan_prod(v[0], l);
    if (NV == 2) v[NV - 1] = wave_scan_prod(v[NV - 1], l) * readlane_d(v[0], 63);
}

// Index idx = l + 64 s < K holds T, G, 1/delta_old and 1/dref; returns delta_new.
// The chain  bd_h = b_h + (0.5 / dref_h) F_h T_h,  dn_h = G_h / bd_h,  F_{h+1} = F_h dn_h / dold_h
// (F_0 = 1, b_0 = bd1, b_h = bd2) is a linear recurrence in y_h = 1 / F_h:
//   y_{h+1} = alpha_h y_h + beta_h,  alpha_h = b_h dold_h / G_h,  beta_h = c_h dold_h / G_h,
// c_h = (0.5 / dref_h) T_h, and dn_h = G_h y_h / (b_h y_h + c_h).  The affine maps compose by a
// wave scan (log2 steps) instead of K dependent steps of lane reads (measured 48.7 us per
// iteration at c4, a serial chain on the critical path).  NV = 2: index l + 64 of the second
// slice composes with the first slice's total map (lane 63).  Every term is positive, so the
// reassociation moves the result by a few ulps only (dc:157-163).
__device__ __forceinline__ void affine_scan(double &A, double &B, int l) {   // inclusive, lane 0 first
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double Ap = __shfl_up(A, o, 64), Bp = __shfl_up(B, o, 64);
        if (l >= o) {
            B = fma(A, Bp, B);
            A = A * Ap;
        }
    }
}
template <int NV>
__device__ __forceinline__ void delta_chain(const Dims &d, int l, const double (&T)[NV], const double (&G)[NV],
                                            const double (&idold)[NV], const double (&idref)[NV], double (&dnew)[NV]) {
    double bh[NV], c[NV], A[NV], B[NV];
    bool act[NV];
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        const int idx = l + 64 * s;
        act[s] = idx < d.K;
        bh[s] = (idx == 0) ? d.bd1 : d.bd2;
        c[s] = (0.5 * idref[s]) * T[s];
        const double inv = 1.0 / (idold[s] * G[s]);              // dold_h / G_h
        A[s] = act[s] ? bh[s] * inv : 1.0;                        // identity map on idle indices
        B[s] = act[s] ? c[s] * inv : 0.0;
        affine_scan(A[s], B[s], l);
    }
    if (NV == 2) {   // the second slice after the whole first one
        const double A0 = readlane_d(A[0], 63), B0 = readlane_d(B[0], 63);
        B[NV - 1] = fma(A[NV - 1], B0, B[NV - 1]);
        A[NV - 1] = A[NV - 1] * A0;
    }
    double yin[NV];
#pragma unroll
    for (int s = 0; s < NV; ++s) yin[s] = A[s] + B[s];            // y_{idx+1} (y_0 = 1)
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        const double yprev = __shfl_up(yin[s], 1, 64);
        const double y = (l == 0) ? (s == 0 ? 1.0 : readlane_d(yin[0], 63)) : yprev;   // y_idx
        dnew[s] = act[s] ? G[s] * y / fma(bh[s], y, c[s]) : 1.0;
    }
}

// P == 1 (Q14): T_h = (sum_{l>=h} tau_l)(sum_{l>=h} s_l) of shard m's incoming tau and column sums
template <int KW, int NV>
__device__ __forceinline__ void rate_sums_p1(const Dims &d, const double *__restrict__ sall,
                                             const double *__restrict__ tau_in, int m, int l, double (&T)[NV]) {
    double ts[NV], ss[NV];
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        const int idx = l + 64 * s, ik = idx < KW ? idx : 0;
        const bool act = idx < d.K;
        ts[s] = act ? tau_in[(size_t)m * KW + ik] : 0.0;
        ss[s] = act ? sall[sall_off(d, m, KW) + ik] : 0.0;
    }
    suffix_sum_nv<NV>(ts, l);
    suffix_sum_nv<NV>(ss, l);
#pragma unroll
    for (int s = 0; s < NV; ++s) T[s] = ts[s] * ss[s];
}

// one wave = one global shard m, lane t (< 64 active); delta / tau rows of KW, NV = KW / 64
// (at least 1) indices per lane.  sall holds the column sums of the iteration the chain
// updates, left by an earlier launch.
template <int KW>
__device__ __forceinline__ void delta_shard(const Dims &d, const double *__restrict__ sall,
                                            const double *__restrict__ delta_in, const double *__restrict__ tau_in,
                                            double *__restrict__ delta_out, double *__restrict__ tau_out,
                                            const DrawsDev &dr, int64_t iter, int m, int t) {
    constexpr int NV = KW > 64 ? KW / 64 : 1;
    if (t < 64) {
        const int l = t;
        if (KW > KP || d.K >= 2) {
            double d0[NV], T0[NV], G0[NV], id0[NV], d0new[NV];
#pragma unroll
            for (int s = 0; s < NV; ++s) {
                const int idx = l + 64 * s, ik = idx < KW ? idx : 0;
                const bool act = idx < d.K;
                d0[s] = act ? delta_in[ik] : 1.0;
                T0[s] = act ? tau_in[ik] * sall[sall_off(d, 0, KW) + ik] : 0.0;
                G0[s] = act ? delta_G(d, dr, iter, 0, idx) : 1.0;
                id0[s] = 1.0 / d0[s];
            }
            if (d.P == 1) rate_sums_p1<KW, NV>(d, sall, tau_in, 0, l, T0);   // Q14
            else suffix_sum_nv<NV>(T0, l);
            delta_chain<NV>(d, l, T0, G0, id0, id0, d0new);   // shard 1 (index 0), its own pre-update delta_h
            double dm[NV];
#pragma unroll
            for (int s = 0; s < NV; ++s) dm[s] = d0new[s];
            if (m != 0) {
                double Tm[NV], Gm[NV], idold[NV], idref[NV];
#pragma unroll
                for (int s = 0; s < NV; ++s) {
                    const int idx = l + 64 * s, ik = idx < KW ? idx : 0;
                    const bool act = idx < d.K;
                    const size_t o = (size_t)m * KW + ik;
                    const double dold = act ? delta_in[o] : 1.0;
                    Tm[s] = act ? tau_in[o] * sall[sall_off(d, m, KW) + ik] : 0.0;
                    Gm[s] = act ? delta_G(d, dr, iter, m, idx) : 1.0;
                    idold[s] = 1.0 / dold;
                    idref[s] = (idx == 0) ? idold[s] : 1.0 / d0new[s];   // delta(1,:,m) | delta(h) (Q4)
                }
                if (d.P == 1) rate_sums_p1<KW, NV>(d, sall, tau_in, m, l, Tm);   // Q14
                else suffix_sum_nv<NV>(Tm, l);
                delta_chain<NV>(d, l, Tm, Gm, idold, idref, dm);
            }
            double tm[NV];
#pragma unroll
            for (int s = 0; s < NV; ++s) tm[s] = (l + 64 * s < d.K) ? dm[s] : 1.0;
            scan_prod_nv<NV>(tm, l);                                     // tauh = cumprod(delta)
#pragma unroll
            for (int s = 0; s < NV; ++s) {
                const int idx = l + 64 * s;
                const bool act = idx < d.K;
                const size_t o = (size_t)m * KW + idx;
                if (idx < KW) {
                    delta_out[o] = act ? dm[s] : delta_in[o];
                    tau_out[o] = act ? tm[s] : tau_in[o];
                }
            }
        } else {   // K == 1 (narrow only)
            if (l == 0) {
                double prefix = 1.0, dnew = 0.0;
                for (int mm = 0; mm <= m; ++mm) {
                    const double dold = delta_in[(size_t)mm * KW];
                    const double tused = prefix * dold;
                    const double smm = sall[sall_off(d, mm, KW)];
                    const double bd = d.bd1 + (0.5 * (1.0 / dold)) * (tused * smm);
                    dnew = (1.0 / bd) * delta_G(d, dr, iter, mm, 0);
                    prefix = prefix * dnew;
                }
                delta_out[(size_t)m * KW] = dnew;
                tau_out[(size_t)m * KW] = prefix;
            }
            if (l >= 1 && l < KW) {
                delta_out[(size_t)m * KW + l] = delta_in[(size_t)m * KW + l];
                tau_out[(size_t)m * KW + l] = tau_in[(size_t)m * KW + l];
            }
        }
    }
}

}  // namespace dcfm
