// The residual-precision update (divideconquer.m:168-171), stated once for every kernel that runs it:
//     Ytil = Yd(:,:,m) - eta(:,:,m)*Lambda(:,:,m)';
//     ps(:,:,m) = gamrnd(as + 0.5*n, 1./(bs + 0.5*sum(Ytil.^2)));
//     Omega(:,:,m) = diag(1./ps(:,:,m));
//   ps_omega_store   dc:170-171 from a row's SS_j and its standard gamma variate: the loading-row kernels
//                    (SS_j by the identity, lambda.h and kernels_wide.hip) and the three residual paths
//   ss_identity_reject  the guard: may the identity's SS_j be used for this row?
//   resid_chunk, resid_lanesum  dc:169 as written for 16 rows i x 16 NH loading rows, fp64 MFMA
//   resid_rows8      K <= 32: a wave's 8 loading rows inside k_lambda (the guard's fallback there)
//   resid_tile       a block's 32 loading rows: k_resid, k_resid_flagged (resid.hip)
// k_resid64 (resid.hip, K <= 32 exact mode) runs resid_chunk on 64 loading rows with its own staging.
#pragma once
#include "dcfm_internal.h"
#include "linalg.h"

namespace dcfm {

// dc:170-171 (Q1: Omega holds 1 / ps).  Plain stores: ps and omega are read by later launches only
__device__ __forceinline__ void ps_omega_store(const Dims &d, double SS, double Gps, double *ps, double *omega,
                                               size_t at) {   // at: the row's index in ps, omega [G][PP]
    const double psn = (1.0 / (d.bs + 0.5 * SS)) * Gps;
    ps[at] = psn;
    omega[at] = 1.0 / psn;
}
// the same with the sample save of dc:185-186 (k_lambda on a saved iteration): the omega just stored
// goes into row a of the open assembly batch, what k_save would read back and add.  The row's one
// writer of omega is its one writer of wsum[a], once per sample
__device__ __forceinline__ void ps_omega_store(const Dims &d, double SS, double Gps, double *ps, double *omega,
                                               size_t at, const SaveArgs &sv, size_t a) {
    const double psn = (1.0 / (d.bs + 0.5 * SS)) * Gps;
    const double w = 1.0 / psn;
    ps[at] = psn;
    omega[at] = w;
    if (sv.Lb) {
        sv.wsum[a] += w;
        if (sv.wslot) sv.wslot[a * sv.B + sv.slot] = w;
    }
}

// ---- guard of the SS identity.  The loading-row kernels form SS_j = yy_j - 2 lambda_j.C_j + lambda_j E
//      lambda_j' without a Y pass; its rounding error is ~ kappa_j eps, kappa_j = (the magnitudes it sums) /
//      SS_j, where the direct residual's is ~ sqrt(kappa_j) eps.  Two bounds on those magnitudes, the larger
//      taken:
//      * as computed: yy_j + mag_j, mag_j = (|w|^2 + sum_r Plam_jr x_r^2 + 2 sum_r |w_r v_r|) / ps_j (narrow;
//        wide: 2 sum_r |x_r C_jr| for the last term), with |w|^2 weighted by 1 + c_j, c_j = max_k Q_kk /
//        L_kk^2 (>= 1, scale-invariant): w = L'x holds only to the back solve's backward error, which grows
//        with the elimination's loss of the diagonal;
//      * a priori: yy_j + 2 sum_k |x_k C_jk| + |x|'|E||x| <= (sqrt(yy_j) + sabs_j)^2, sabs_j = sum_k |x_k|
//        sqrt(E_kk) (|C_jk| <= sqrt(E_kk yy_j) and |E_kl| <= sqrt(E_kk E_ll), E a Gram matrix).
//      Beyond kappa_max (or SS_j <= 0) the row takes dc:169's residual instead: K <= 32 the wave's 8 rows
//      in the same launch (resid_rows8), K > 32 the row's 32-row tile in k_resid_flagged.
//      sqrt(yy_j) as v * rsq(v) from the hardware estimate (a bound needs no correct rounding; the factor
//      1.01 covers its error).  A zero yy_j makes that product NaN, and fmax returns its other argument:
//      the a-priori bound would drop out unseen, so the accepting conjunction asks for yy_j > 0 itself (a
//      zero, negative or NaN yy_j takes the residual; preprocessing drops zero columns, so no sweep pays).
//      kappa_max = 0 rejects every row (DCFM_FLAG_GUARD_ALL), infinity none with SS_j > 0 and yy_j > 0.
#ifndef DCFM_KAPPA_MAX
#define DCFM_KAPPA_MAX 1e3
#endif
constexpr double KAPPA_IDENTITY_MAX = DCFM_KAPPA_MAX;
__device__ __forceinline__ bool ss_identity_reject(double yy, double SS, double mag, double sabs, double kappa_max) {
    const double rt = 1.01 * (yy * __builtin_amdgcn_rsq(yy) + sabs);
    const double num = fmax(rt * rt, 1.01 * (yy + mag));
    return !(SS > 0.0 && yy > 0.0 && num <= kappa_max * SS);
}

// ---- dc:169 as written, fp64 MFMA v_mfma_f64_16x16x4.  One chunk = rows i0 .. i0+15 of i against NH tiles
//      of 16 loading rows: the Y values are the accumulator input and eta the A operand under the
//      instruction's neg modifier (D = Y - eta Lambda', the subtraction of dc:169 inside the accumulation),
//      A[i = lane&15][k], B[k][j = lane&15] with k = 8t + 2q (+1), so both operands are 16-byte pairs:
//      eta_at(t) = eta[i0 + c][8t + 2q, +1] (a callable: the operand is formed where the caller's staging
//      has it), lb[h][t] = Lambda[tile h's row c][8t + 2q, +1].  Lane (c, q) then holds Ytil for rows
//      row0 + 4v, row0 = i0 + q, of tile h's loading row c and squares the data rows (< n) into ss[h].
//      Each accumulator takes its products in the order t ascending, .x then .y; the NH chains are
//      independent.
__device__ __forceinline__ d2 eta_pair(const Dims &d, d2 x, d2 z) {
    return d2{eta_of(d.sr, d.s1r, x.x, z.x), eta_of(d.sr, d.s1r, x.y, z.y)};
}
template <int NT, int NH, class EtaAt>
__device__ __forceinline__ void resid_chunk(const d4 (&y)[NH], EtaAt eta_at, const d2 (&lb)[NH][NT], int row0, int n,
                                            double (&ss)[NH]) {
    d4 acc[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) acc[h] = y[h];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const d2 e = eta_at(t);
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[h] = mfma16x16x4_na(e.x, lb[h][t].x, acc[h]);
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[h] = mfma16x16x4_na(e.y, lb[h][t].y, acc[h]);
    }
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int v = 0; v < 4; ++v)
            ss[h] = (row0 + 4 * v < n) ? fma(acc[h][v], acc[h][v], ss[h]) : ss[h];   // padding rows: not data
}
// a loading row's 4 lanes (q = 0..3) after the last chunk: (q0 + q1) + (q2 + q3), in every lane
template <int NH>
__device__ __forceinline__ void resid_lanesum(double (&ss)[NH]) {
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        ss[h] += xor16_d(ss[h]);
        ss[h] += xor32_d(ss[h]);
    }
}

// K <= 32, inside k_lambda: the wave's 8 loading rows j0 .. j0+7 over every chunk of i.  B = the rows'
// Lambda from k_lambda's LDS image Lm (columns 8..15 of the tile zero), Gps_c the variate of row j0 + c;
// sv: the omega half of the sample save on a saved iteration (ps_omega_store)
constexpr int LAM_ROWS = 8;   // loading rows per wave of k_lambda
__device__ __forceinline__ void resid_rows8(const Dims &d, const double *__restrict__ Y,
                                            const double *__restrict__ X, const double *__restrict__ Z,
                                            const double (*Lm)[KP + 1], double Gps_c, int m, int j0, int lane,
                                            double *__restrict__ ps, double *__restrict__ omega, const SaveArgs &sv) {
    constexpr int NT = KP / 8;
    const int c = lane & 15, q = lane >> 4;
    const bool col = c < LAM_ROWS && j0 + c < d.P;
    d2 lb[1][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        lb[0][t].x = col ? Lm[c][8 * t + 2 * q] : 0.0;
        lb[0][t].y = col ? Lm[c][8 * t + 2 * q + 1] : 0.0;
    }
    const double *Ym = Y + (size_t)m * d.NP * d.PP + (col ? j0 + c : 0);
    const double *Zm = Z + (size_t)m * d.NP * KP + 2 * q;
    double ss[1] = {0.0};
    for (int i0 = 0; i0 < d.NP; i0 += 16) {
        d4 y[1];
#pragma unroll
        for (int v = 0; v < 4; ++v) y[0][v] = col ? Ym[(size_t)(i0 + q + 4 * v) * d.PP] : 0.0;
        const double *xr = X + (size_t)(i0 + c) * KP + 2 * q, *zr = Zm + (size_t)(i0 + c) * KP;
        resid_chunk(y, [&](int t) {
            return eta_pair(d, *reinterpret_cast<const d2 *>(xr + 8 * t), *reinterpret_cast<const d2 *>(zr + 8 * t));
        }, lb, i0 + q, d.n, ss);
    }
    resid_lanesum(ss);
    if (q == 0 && col)
        ps_omega_store(d, ss[0], Gps_c, ps, omega, (uint32_t)(m * d.PP + j0 + c), sv, (size_t)(d.shard0 + m) * d.P + j0 + c);
}

// Loading rows j0 .. j0+31 of shard m by a block of 256 threads = 4 waves, which split the chunks of i;
// a wave runs two column tiles per chunk, Lambda register-resident.  The 4 lanes of a row, then the 4
// waves (through red), are summed in a fixed order; Gps in the LamDraws layout [G][P]
template <int KW>
__device__ __forceinline__ void resid_tile(const Dims &d, const double *__restrict__ Y, const double *__restrict__ X,
                                           const double *__restrict__ Z, const double *__restrict__ Lam,
                                           const double *__restrict__ Gps, double *__restrict__ ps,
                                           double *__restrict__ omega, int m, int j0, double (*red)[32]) {
    constexpr int NT = KW / 8;                  // k steps of 8 (two MFMAs each)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const double *Ym = Y + (size_t)m * d.NP * d.PP;
    const double *Zm = Z + (size_t)m * d.NP * KW;
    d2 lb[2][NT];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < NT; ++t)
            lb[h][t] = *reinterpret_cast<const d2 *>(Lam + ((size_t)m * d.PP + j0 + 16 * h + c) * KW + 8 * t + 2 * q);
    double ss[2] = {0.0, 0.0};
    const int nch = d.NP / 16;
    for (int ch = w; ch < nch; ch += 4) {
        const int i0 = 16 * ch;
        d4 y[2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) y[h][v] = Ym[(size_t)(i0 + q + 4 * v) * d.PP + j0 + 16 * h + c];
        const double *xr = X + (size_t)(i0 + c) * KW + 2 * q;
        const double *zr = Zm + (size_t)(i0 + c) * KW + 2 * q;
        resid_chunk(y, [&](int t) {
            return eta_pair(d, *reinterpret_cast<const d2 *>(xr + 8 * t), *reinterpret_cast<const d2 *>(zr + 8 * t));
        }, lb, i0 + q, d.n, ss);
    }
    resid_lanesum(ss);
    if (q == 0) {
        red[w][c] = ss[0];
        red[w][16 + c] = ss[1];
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        const int j = j0 + threadIdx.x;
        const double SS = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (j < d.P) ps_omega_store(d, SS, Gps[(size_t)m * d.P + j], ps, omega, (size_t)m * d.PP + j);
    }
}

}  // namespace dcfm
