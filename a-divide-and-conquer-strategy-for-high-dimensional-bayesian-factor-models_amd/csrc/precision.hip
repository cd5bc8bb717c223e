// Per-sample posterior draws of V' Sigma(s)^{-1} V and log det Sigma(s) for a caller-chosen block of probe
// vectors (dcfm_set_precision_probes / dcfm_get_precision_draws).
//
// dcfm_sigma_solve gives Sigmaout^{-1} B, the inverse of the posterior mean.  The posterior of anything that
// goes through the inverse -- a Mahalanobis distance, a discriminant score, minimum-variance weights, the
// held-out Gaussian log density -- needs Sigma(s)^{-1} per saved sample, and none needs Sigma(s) formed, a
// p x p factorisation or an iteration: Sigma(s) = D + rho Lbar Lbar' with D = blockdiag(D_m),
// D_m = (1 - rho) L_m L_m' + Omega_m (dc:182-192), is block-diagonal plus rank K, so two nested Woodbury
// steps do it.  With V_m the shard's rows of V, a = 1 - rho and the shard's weighted Gram
//   [G_m U_m; U_m' d_m] = [L_m V_m]' Omega_m^{-1} [L_m V_m]                     (width w = K + nv)
//   B_m = I + a G_m  (SPD for every rho in [0, 1]),
//   H_m = B_m^{-1} G_m = L_m' D_m^{-1} L_m,   F_m = B_m^{-1} U_m = L_m' D_m^{-1} V_m,
//   q_m = d_m - a U_m' F_m = V_m' D_m^{-1} V_m,   ld_m = sum_j log omega_mj + log det B_m,
// and over the shards F = sum F_m, H = sum H_m, q = sum q_m, S = I + rho H (SPD):
//   V' Sigma(s)^{-1} V = q - rho F' S^{-1} F,      log det Sigma(s) = sum_m ld_m + log det S.
// B_m and S keep the identity unscaled, so rho = 0 and rho = 1 need no special case.
//
// k_precision runs behind the sample save (and k_probes) on the sweep stream, slices x G blocks:
//   1. every block reduces a fixed slice of a shard's rows into the lower 16x16 tiles of the weighted Gram
//      with v_mfma_f64_16x16x4 (the rows staged in LDS 32 at a time, [L | V] padded to 16 columns with
//      zeros; a wave holds every fourth tile, at most 14, in accumulators) and sum log omega;
//   2. the shard's last slice block (handoff.h's ticket) adds the slices in slice order, inverts B_m in
//      LDS (in-place Gauss-Jordan: K pivots in index order, four a pass, no pivot search and no data-dependent trip
//      count, so a NaN state runs through to NaN draws; log det B_m = the sum of the pivots' logs), forms
//      [H_m | F_m] = B_m^{-1} [G_m | U_m] 16 columns at a time, q_m and ld_m and stores the term;
//   3. the last shard block of a group of PROBE_FAN shards adds its shards' terms in shard order and the
//      last group block the groups' in group order, as k_probes; one rank then inverts S the same way
//      and writes q - rho F' S^{-1} F (one triangle, mirrored) and the log det; several ranks store their
//      sum [H_r | F_r | q_r | ld_r], which the read-out gathers in one collective over all draws, adds in
//      rank order and finishes on the host with a K x K Cholesky.
// No floating-point atomics and fixed orders throughout: the same inputs give the same bits.
//
// Operating point: the Gram is the only stage whose flops grow with p (p w^2) and maps onto MFMA tiles
// of the padded panel directly; the K x K stages are plain fp64 FMA over LDS (K^3 per inversion, K^2 w
// per product, by one block per shard): DESIGN.md 4e has the measurements.
#include "handle.h"
#include "handoff.h"
#include "tile_linalg.h"
#include "gj.h"

namespace dcfm {

constexpr int PREC_ROWS = 32;     // loading rows staged per step
constexpr int PREC_TPW = 14;      // tiles of a wave: ceil(55 / 4), 55 = the lower tiles of w = 160
static_assert(precision_tiles(KP_MAX, PROBE_NV_MAX) <= 4 * PREC_TPW, "a wave's accumulators hold its tiles");

// doubles of dynamic LDS: the staged rows of stage 1; A (K x K) and a panel (the inversion's column panel in
// its place) of stages 2 and 3; the two K x 32 operands of the closing products
inline size_t precision_lds_doubles(int K, int nv) {
    const size_t wp = (size_t)(K + nv + 15) / 16 * 16, s1 = PREC_ROWS * wp + PREC_ROWS,
                 s2 = (size_t)K * K + (size_t)K * PREC_PANEL + 2, s3 = 2 * (size_t)K * PROBE_NV_MAX;
    return std::max(s1, std::max(s2, s3));
}

// acc[i] = the sum over k < count of src[k * stride + e0 + 256 i] in k order, i < FE, for the elements below n.
// The agent-scope loads are independent of one another and FE x FK of them are in flight per thread before
// the first is added (fold_terms of probes.hip: one at a time is one L2 round trip each); a load past the
// count or past n re-reads a valid address and is dropped
constexpr int PREC_FE = 4;
__device__ __forceinline__ void fold_sum(const double *src, int count, size_t stride, size_t e0, size_t n,
                                         double (&acc)[PREC_FE]) {
    constexpr int FK = 8;
    size_t e[PREC_FE];
#pragma unroll
    for (int i = 0; i < PREC_FE; ++i) {
        e[i] = e0 + 256 * i < n ? e0 + 256 * i : 0;
        acc[i] = 0.0;
    }
    for (int k0 = 0; k0 < count; k0 += FK) {
        double v[PREC_FE][FK];
#pragma unroll
        for (int u = 0; u < FK; ++u)
#pragma unroll
            for (int i = 0; i < PREC_FE; ++i) v[i][u] = ld_agent(src + (size_t)min(k0 + u, count - 1) * stride + e[i]);
#pragma unroll
        for (int u = 0; u < FK; ++u)
#pragma unroll
            for (int i = 0; i < PREC_FE; ++i)
                if (k0 + u < count) acc[i] += v[i][u];
    }
}

// dst[e] = the sum of `count` terms of ts doubles, src[k * ts + e] over k in k order (agent-scope both ways)
template <bool AGENT>
__device__ __forceinline__ void fold_terms(const double *src, int count, size_t ts, double *dst) {
    for (size_t e0 = threadIdx.x; e0 < ts; e0 += 256 * PREC_FE) {
        double acc[PREC_FE];
        fold_sum(src, count, ts, e0, ts, acc);
#pragma unroll
        for (int i = 0; i < PREC_FE; ++i)
            if (e0 + 256 * i < ts) {
                if (AGENT) st_agent(dst + e0 + 256 * i, acc[i]);
                else dst[e0 + 256 * i] = acc[i];
            }
    }
}

// out(a, b) = base(a, b) - scale * sum_k X(k, a) Y(k, b) for a >= b < nv, mirrored; X and Y are K x nv in
// global memory (ldx, ldy), staged 32 wide into sX, sY; base is nv x nv with rows ldb apart, out nv x nv row-major
template <bool AGENT>
__device__ __forceinline__ void close_quad(const double *X, int ldx, const double *Y, int ldy, int K, int nv, double scale,
                                           const double *base, int ldb, double *out, double *sX, double *sY) {
    const int t = threadIdx.x;
    for (int e = t; e < K * PROBE_NV_MAX; e += 256) {
        const int k = e >> 5, c = e & 31;
        sX[e] = c < nv ? ld_agent(X + (size_t)k * ldx + c) : 0.0;
        sY[e] = c < nv ? ld_agent(Y + (size_t)k * ldy + c) : 0.0;
    }
    __syncthreads();
    for (int e = t; e < nv * nv; e += 256) {
        const int a = e / nv, b = e % nv;
        if (a < b) continue;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc = fma(sX[k * PROBE_NV_MAX + a], sY[k * PROBE_NV_MAX + b], acc);
        const double v = fma(-scale, acc, ld_agent(base + (size_t)a * ldb + b));
        if (AGENT) {
            st_agent(out + a * nv + b, v);
            st_agent(out + b * nv + a, v);
        } else {
            out[a * nv + b] = v;
            out[b * nv + a] = v;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_precision(const double *__restrict__ Lam, const double *__restrict__ omega,
                                                   const double *__restrict__ V, int P, int PP, int KW, int K, int G,
                                                   int nv, double rho, int form, double *part, double *gram,
                                                   double *term, double *gterm, double *rsum, double *xs,
                                                   unsigned *ticket, double *__restrict__ draw,
                                                   double *__restrict__ binv,
                                                   const unsigned char *__restrict__ obs, double *__restrict__ sinv) {
    extern __shared__ __align__(16) double dyn[];
    __shared__ double red[256];
    __shared__ unsigned flag;
    const int sl = blockIdx.x, S = gridDim.x, m = blockIdx.y, t = threadIdx.x;
    const int wave = t >> 6, lane = t & 63, li = lane & 15, kq = lane >> 4;
    const int w = K + nv, nbt = (w + 15) / 16, wp = 16 * nbt, ntl = nbt * (nbt + 1) / 2;
    const size_t ps = (size_t)ntl * 256 + 1, ts = (size_t)K * w + (size_t)nv * nv + 1;
    const int j0 = (int)((long long)P * sl / S), j1 = (int)((long long)P * (sl + 1) / S);
    const double *Lm = Lam + (size_t)m * PP * KW, *Vm = V + (size_t)m * P * nv, *om = omega + (size_t)m * PP;

    // ---- 1. the slice's partial of [L | V]' Omega^{-1} [L | V]: tile wave + 4 u of the lower triangle
    double *sX = dyn, *sW = dyn + PREC_ROWS * wp;
    int cI[PREC_TPW], cJ[PREC_TPW];
    d4 acc[PREC_TPW];
    const int nmine = ntl > wave ? (ntl - wave + 3) / 4 : 0;
#pragma unroll
    for (int u = 0; u < PREC_TPW; ++u) {
        int a = 0, b = 0;
        if (u < nmine) tile::tri_pair(wave + 4 * u, a, b);
        cI[u] = 16 * a + li;
        cJ[u] = 16 * b + li;
        acc[u] = d4{0.0, 0.0, 0.0, 0.0};
    }
    double lw = 0.0;
    for (int r0 = j0; r0 < j1; r0 += PREC_ROWS) {
        const int nr = min(PREC_ROWS, j1 - r0), nr4 = (nr + 3) & ~3;
        for (int e = t; e < nr4 * wp; e += 256) {
            const int r = e / wp, c = e - r * wp;
            double v = 0.0;
            if (r < nr && c < K) v = Lm[(size_t)(r0 + r) * KW + c];
            else if (r < nr && c < w) v = Vm[(size_t)(r0 + r) * nv + (c - K)];
            sX[e] = v;
        }
        if (t < nr4) {
            // predict.hip's mask: an unobserved row takes weight 0 and log term 0 by selects (its omega need not be
            // invertible); obs null: every row of the slice counts
            const bool on = t < nr && (!obs || obs[(size_t)m * P + r0 + t] != 0);
            const double o = t < nr ? om[r0 + t] : 1.0;
            sW[t] = on ? 1.0 / o : 0.0;
            lw += on ? log(o) : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < nr4; r += 4) {
            const double *xr = sX + (r + kq) * wp;
            const double wt = sW[r + kq];
#pragma unroll
            for (int u = 0; u < PREC_TPW; ++u)
                if (u < nmine) acc[u] = mfma16x16x4(wt * xr[cI[u]], xr[cJ[u]], acc[u]);
        }
        __syncthreads();
    }
    double *mine = part + ((size_t)m * S + sl) * ps;
#pragma unroll
    for (int u = 0; u < PREC_TPW; ++u)
        if (u < nmine)
#pragma unroll
            for (int g = 0; g < 4; ++g) st_agent(mine + (size_t)(wave + 4 * u) * 256 + g * 64 + lane, acc[u][g]);
    red[t] = lw;                                          // sum log omega of the slice: a fixed tree
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) st_agent(mine + (size_t)ntl * 256, red[0]);

    // ---- 2. the shard's last slice block: the slices in slice order, then the shard's term
    if (!last_arrival(ticket + m, S, &flag)) return;
    double *Mg = gram + (size_t)m * w * w, *tm = term + (size_t)m * ts;
    const double *pm = part + (size_t)m * S * ps;
    for (size_t e0 = t; e0 < ps; e0 += 256 * PREC_FE) {
        double fs[PREC_FE];
        fold_sum(pm, S, ps, e0, ps, fs);
#pragma unroll
        for (int i = 0; i < PREC_FE; ++i) {
            const size_t e = e0 + 256 * i;
            if (e >= ps) continue;
            if (e == (size_t)ntl * 256) {
                red[0] = fs[i];
                continue;
            }
            int a, b;
            tile::tri_pair((int)(e >> 8), a, b);
            const int ln = (int)(e & 63), row = 16 * a + (ln >> 4) + 4 * (int)((e >> 6) & 3), col = 16 * b + (ln & 15);
            if (row < w && col <= row) {                  // D[row = q + 4 g][col = lane & 15] of the tile
                st_agent(Mg + (size_t)row * w + col, fs[i]);
                st_agent(Mg + (size_t)col * w + row, fs[i]);
            }
        }
    }
    stores_done();
    const double slw = red[0];
    double *A = dyn, *sP = dyn + K * K, *Cc = sP + (K & 1);   // Cc: 16-byte aligned inside the idle panel
    load_shifted(A, K, Mg, w, 1.0 - rho);                 // B_m = I + (1 - rho) G_m
    const double ldB = gj_invert(A, K, Cc);
    if (binv)                                             // loglik.hip keeps B_m^{-1} (read by a later launch)
        for (int e = t; e < K * K; e += 256) binv[(size_t)m * K * K + e] = A[e];
    mat_apply(A, K, Mg, w, w, tm, w, sP);                 // [H_m | F_m] = B^{-1} [G_m | U_m]
    stores_done();
    close_quad<true>(Mg + K, w, tm + K, w, K, nv, 1.0 - rho, Mg + (size_t)K * w + K, w, tm + (size_t)K * w, dyn,
                     dyn + K * PROBE_NV_MAX);         // q_m = d_m - (1 - rho) U_m' F_m
    if (t == 0) st_agent(tm + ts - 1, slw + ldB);

    // ---- 3. the last shard block of a group of PROBE_FAN shards: its shards in shard order
    const int gi = m / PROBE_FAN, ng = (G + PROBE_FAN - 1) / PROBE_FAN, cnt = min(PROBE_FAN, G - gi * PROBE_FAN);
    if (!last_arrival(ticket + G + gi, cnt, &flag)) return;
    fold_terms<true>(term + (size_t)gi * PROBE_FAN * ts, cnt, ts, gterm + (size_t)gi * ts);
    // the rank's last group block: the groups in group order
    if (!last_arrival(ticket + G + ng, ng, &flag)) return;
    if (!form) {                                          // several ranks: the rank's sum for the read-out
        fold_terms<false>(gterm, ng, ts, draw);
        return;
    }
    fold_terms<true>(gterm, ng, ts, rsum);
    stores_done();
    load_shifted(A, K, rsum, w, rho);                     // S = I + rho H
    const double ldS = gj_invert(A, K, Cc);
    if (sinv)                                             // predict.hip keeps S^{-1} (read by a later launch)
        for (int e = t; e < K * K; e += 256) sinv[e] = A[e];
    mat_apply(A, K, rsum + K, w, nv, xs, nv, sP);         // S^{-1} F
    stores_done();
    close_quad<false>(rsum + K, w, xs, nv, K, nv, rho, rsum + (size_t)K * w, nv, draw, dyn, dyn + K * PROBE_NV_MAX);
    if (t == 0) draw[nv * nv] = ld_agent(rsum + ts - 1) + ldS;
}

void launch_precision(const Dims &d, const Bufs &b, const Precision &pr, int64_t s, hipStream_t st) {
    hipLaunchKernelGGL(k_precision, dim3(pr.slices, d.G), dim3(256), pr.lds, st, b.Lam, b.omega, pr.V, d.P, d.PP, d.kp,
                       d.K, d.G, pr.nv, d.rho, d.coll ? 0 : 1, pr.part, pr.gram, pr.term, pr.gterm, pr.rsum, pr.xs,
                       pr.ticket, pr.draws + (size_t)s * pr.slot, nullptr, nullptr, nullptr);
}

// predict.hip: the one-rank form with pr.V = the new rows, the weight masked by obs [G][P]: draw = [q (nv x nv) | ld]
// of Sigma_AA(s), sinv = S^{-1}; pr.term, pr.rsum and pr.xs keep [H_m | F_m], [H | F] and S^{-1} F for the next launch
void launch_precision_masked(const Dims &d, const Bufs &b, const Precision &pr, const unsigned char *obs, double *sinv,
                             double *draw, hipStream_t st) {
    hipLaunchKernelGGL(k_precision, dim3(pr.slices, d.G), dim3(256), pr.lds, st, b.Lam, b.omega, pr.V, d.P, d.PP, d.kp,
                       d.K, d.G, pr.nv, d.rho, 1, pr.part, pr.gram, pr.term, pr.gterm, pr.rsum, pr.xs, pr.ticket, draw,
                       nullptr, obs, sinv);
}

// loglik.hip: the stages at nv = 0 -- out = the rank's sum [H_r (K x K) | ld_r], binv [G][K][K] the shards' B_m^{-1}
void launch_precision_terms(const Dims &d, const Bufs &b, const Precision &pr, double *binv, double *out, hipStream_t st) {
    hipLaunchKernelGGL(k_precision, dim3(pr.slices, d.G), dim3(256), pr.lds, st, b.Lam, b.omega, nullptr, d.P, d.PP, d.kp,
                       d.K, d.G, 0, d.rho, 0, pr.part, pr.gram, pr.term, pr.gterm, pr.rsum, pr.xs, pr.ticket, out, binv,
                       nullptr, nullptr);
}

static int prec_groups(int G) { return (G + PROBE_FAN - 1) / PROBE_FAN; }
static size_t prec_ticket_doubles(int G) { return ((size_t)G + prec_groups(G) + 1 + 1) / 2; }

// k_precision's scratch for nv probes: [ticket | part | gram | term, gterm, rsum | xs] (dcfm_internal.h has the
// sizes); the caller zeroes the first precision_ticket_doubles (the tickets start at 0)
size_t precision_ticket_doubles(const Dims &d) { return prec_ticket_doubles(d.G); }
size_t precision_scratch_doubles(const Dims &d, int nv) {
    const size_t w = (size_t)d.K + nv, ts = (size_t)d.K * w + (size_t)nv * nv + 1, ps = (size_t)precision_tiles(d.K, nv) * 256 + 1;
    return prec_ticket_doubles(d.G) + (size_t)d.G * precision_slices(d.G, d.P, d.K, nv) * ps + (size_t)d.G * w * w +
           ((size_t)d.G + prec_groups(d.G) + 1) * ts + (size_t)d.K * nv;
}
void precision_scratch_carve(const Dims &d, int nv, double *mem, Precision &pr) {
    const size_t w = (size_t)d.K + nv, ts = (size_t)d.K * w + (size_t)nv * nv + 1, ps = (size_t)precision_tiles(d.K, nv) * 256 + 1;
    pr.nv = nv;
    pr.slices = precision_slices(d.G, d.P, d.K, nv);
    pr.lds = precision_lds_doubles(d.K, nv) * sizeof(double);
    pr.ticket = reinterpret_cast<unsigned *>(mem);
    pr.part = mem + prec_ticket_doubles(d.G);
    pr.gram = pr.part + (size_t)d.G * pr.slices * ps;
    pr.term = pr.gram + (size_t)d.G * w * w;
    pr.gterm = pr.term + (size_t)d.G * ts;
    pr.rsum = pr.gterm + (size_t)prec_groups(d.G) * ts;
    pr.xs = pr.rsum + ts;
}
// the largest footprint (K = 128, nv = 32: 146 KB) passes the default limit of dynamic LDS; the attribute
// belongs to the kernel, not the handle, so it is set to that whatever this handle's K
hipError_t precision_setup() {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k_precision), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(precision_lds_doubles(KP_MAX, PROBE_NV_MAX) * sizeof(double)));
}

}  // namespace dcfm

// Host close of the several-rank read-out: t = [H | F (K x w) | q (nv x nv) | ld] summed over the ranks;
// S = I + rho H = R R' (plain Cholesky of the lower triangle), T = R^{-1} F, Q = q - rho T'T (one triangle,
// mirrored), returns ld + 2 sum log diag R.  Fixed trip counts: a NaN runs through
static double host_close(const double *t, int K, int nv, double rho, double *Q) {
    const int w = K + nv;
    std::vector<double> R((size_t)K * K), T((size_t)K * std::max(nv, 1));
    double ld = t[(size_t)K * w + (size_t)nv * nv];
    for (int j = 0; j < K; ++j) {
        for (int i = j; i < K; ++i) {
            double s = std::fma(rho, t[(size_t)i * w + j], i == j ? 1.0 : 0.0);
            for (int k = 0; k < j; ++k) s = std::fma(-R[(size_t)i * K + k], R[(size_t)j * K + k], s);
            R[(size_t)i * K + j] = i == j ? std::sqrt(s) : s / R[(size_t)j * K + j];
        }
        ld += 2.0 * std::log(R[(size_t)j * K + j]);
    }
    for (int c = 0; c < nv; ++c)
        for (int i = 0; i < K; ++i) {
            double s = t[(size_t)i * w + K + c];
            for (int k = 0; k < i; ++k) s = std::fma(-R[(size_t)i * K + k], T[(size_t)k * nv + c], s);
            T[(size_t)i * nv + c] = s / R[(size_t)i * K + i];
        }
    const double *q = t + (size_t)K * w;
    for (int a = 0; a < nv; ++a)
        for (int b = 0; b <= a; ++b) {
            double acc = 0.0;
            for (int k = 0; k < K; ++k) acc = std::fma(T[(size_t)k * nv + a], T[(size_t)k * nv + b], acc);
            Q[a * nv + b] = Q[b * nv + a] = std::fma(-rho, acc, q[a * nv + b]);
        }
    return ld;
}

extern "C" {

int dcfm_set_precision_probes(dcfm_handle *h, const double *V, int32_t nv, int64_t capacity) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    const Dims &d = h->d;
    if (capacity < 0) return fail(h, DCFM_ERR_INVALID, "set_precision_probes: capacity %lld < 0", (long long)capacity);
    if (capacity > 0) {
        if (nv < 0 || nv > PROBE_NV_MAX)
            return fail(h, DCFM_ERR_INVALID, "set_precision_probes: nv = %d outside 0..%d", (int)nv, PROBE_NV_MAX);
        if (!V && nv > 0) return fail(h, DCFM_ERR_INVALID, "null argument");
        for (size_t e = 0; e < (size_t)d.p * nv; ++e)
            if (!std::isfinite(V[e]))
                return fail(h, DCFM_ERR_INVALID, "set_precision_probes: V(%zu, %zu) is not finite", e % d.p + 1, e / d.p + 1);
    }
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (h->prec_mem) (void)hipFree(h->prec_mem);
    h->prec_mem = nullptr;
    h->prec = Precision{};
    h->prec_cap = h->prec_n = 0;
    if (capacity == 0) return DCFM_OK;
    Precision pr{};
    HIPC(h, precision_setup());
    const size_t rows = (size_t)d.G * d.P, w = (size_t)d.K + nv, ts = (size_t)d.K * w + (size_t)nv * nv + 1;
    pr.slot = d.coll ? ts : (size_t)nv * nv + 1;
    const size_t nscr = precision_scratch_doubles(d, nv), nV = rows * nv;
    void *q = nullptr;
    if (hipMalloc(&q, (nscr + nV + (size_t)capacity * pr.slot) * sizeof(double)) != hipSuccess)
        return fail(h, DCFM_ERR_ALLOC, "set_precision_probes: %lld draws of %d probes", (long long)capacity, (int)nv);
    h->prec_mem = static_cast<double *>(q);
    precision_scratch_carve(d, nv, h->prec_mem, pr);
    double *dV = h->prec_mem + nscr;
    pr.V = dV;
    pr.draws = dV + nV;
    HIPC(h, hipMemset(h->prec_mem, 0, precision_ticket_doubles(d) * sizeof(double)));   // tickets start at 0
    if (nV) {   // this rank's rows of V, row-major
        std::vector<double> loc(nV);
        const size_t row0 = (size_t)d.shard0 * d.P;
        for (size_t j = 0; j < rows; ++j)
            for (int c = 0; c < nv; ++c) loc[j * nv + c] = V[(size_t)c * d.p + row0 + j];
        HIPC(h, hipMemcpy(dV, loc.data(), nV * sizeof(double), hipMemcpyHostToDevice));
    }
    h->prec = pr;
    h->prec_cap = capacity;
    return DCFM_OK;
}

int dcfm_get_precision_draws(dcfm_handle *h, double *Q, double *logdet, int64_t *count) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    const Dims &d = h->d;
    const Precision &pr = h->prec;
    int code = count ? DCFM_OK : fail(h, DCFM_ERR_INVALID, "null argument");
    if (code == DCFM_OK) {
        hipError_t e = hipSetDevice(h->cfg.device);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) code = fail(h, DCFM_ERR_HIP, "get_precision_draws: %s", hipGetErrorString(e));
    }
    const size_t S = (size_t)h->prec_n, nv = (size_t)pr.nv, nq = nv * nv, mine = S * pr.slot;
    const bool want = Q || logdet;
    if (!d.coll || S == 0) {   // one rank: the kernel closed the draw.  No draw (on every rank): nothing to gather
        if (code != DCFM_OK) return code;
        *count = h->prec_n;
        if (want && S) {
            std::vector<double> host(mine);
            HIPC(h, hipMemcpy(host.data(), pr.draws, mine * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t s = 0; s < S; ++s) {
                if (Q) std::copy_n(host.data() + s * pr.slot, nq, Q + s * nq);
                if (logdet) logdet[s] = host[s * pr.slot + nq];
            }
        }
        return DCFM_OK;
    }
    // several ranks: every rank's [H_r | F_r | q_r | ld_r] of all draws in one all-gather, summed in rank order
    TRY(agree(h, code));
    *count = h->prec_n;
    const size_t nr = (size_t)d.nranks;
    void *g = nullptr;
    if (hipMalloc(&g, nr * mine * sizeof(double)) != hipSuccess)
        code = fail(h, DCFM_ERR_ALLOC, "get_precision_draws: gather of %zu doubles", nr * mine);
    if (int rc = agree(h, code)) {
        if (g) (void)hipFree(g);
        return rc;
    }
    double *all = static_cast<double *>(g);
    std::vector<double> host(want ? nr * mine : 0);
    int rc = coll_allgather(h, CH_MAIN, pr.draws, all, mine, h->stream);
    if (rc == DCFM_OK && want) {
        const hipError_t e = hipMemcpyAsync(host.data(), all, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) rc = fail(h, DCFM_ERR_HIP, "get_precision_draws: %s", hipGetErrorString(e));
    }
    const hipError_t es = hipStreamSynchronize(h->stream);
    (void)hipFree(all);
    if (rc == DCFM_OK && es != hipSuccess) rc = fail(h, DCFM_ERR_HIP, "get_precision_draws: %s", hipGetErrorString(es));
    if (rc != DCFM_OK || !want) return rc;
    std::vector<double> sum(pr.slot), q(nq);
    for (size_t s = 0; s < S; ++s) {
        std::fill(sum.begin(), sum.end(), 0.0);
        for (size_t r = 0; r < nr; ++r) {
            const double *t = host.data() + (r * S + s) * pr.slot;
            for (size_t e = 0; e < pr.slot; ++e) sum[e] += t[e];
        }
        const double ld = host_close(sum.data(), d.K, pr.nv, d.rho, q.data());
        if (Q) std::copy(q.begin(), q.end(), Q + s * nq);
        if (logdet) logdet[s] = ld;
    }
    return DCFM_OK;
}

}  // extern "C"
