// Conditional prediction of unobserved variables under the posterior (dcfm_set_predict / dcfm_get_predict):
// a new row arrives with the variables of an index set A observed; for every saved sample s the device forms
//   yhat_j(s) = E[(Lambda eta)_j | y_A, Sigma(s)]   (= E[y_j | y_A, Sigma(s)] for j outside A),
//   cv_j(s)   = the predictive variance of a fresh observation of variable j given y_A (= Var[y_j | y_A, Sigma(s)]
//               for j outside A),
//   q(s) = y_A' Sigma_AA(s)^{-1} y_A  and  ld(s) = log det Sigma_AA(s)
// for up to 32 new rows at once (the columns of Y*, p x T) and accumulates sum yhat, sum yhat^2 and sum cv over
// the samples, so that the read-out gives the posterior mean and, by the law of total variance, the posterior
// predictive variance avg_s cv_j(s) + var_s yhat_jt(s).
//
// The recursion is precision.hip's nested Woodbury with the Gram's weight masked: restricting to A only removes
// rows from the weighted Gram, so Sigma_AA(s) is again block-diagonal plus rank K.  With a = 1 - rho, obs the
// 0 / 1 mask, W_m = diag(obs_j / omega_mj), per shard
//   [G_m U_m; . d_m] = [L_m Y*_m]' W_m [L_m Y*_m],  B_m = I + a G_m,  H_m = B_m^{-1} G_m,  F_m = B_m^{-1} U_m,
//   q_m = d_m - a U_m' F_m,  ld_m = sum_{j in A} log omega_mj + log det B_m
// and over the shards H = sum H_m, F = sum F_m, S = I + rho H, R = S^{-1}, X = R F (K x T):
//   q = sum q_m - rho F' X,   ld = sum ld_m + log det S,
//   c_m = F_m - rho H_m X,  c = F - rho H X,  t_m = a c_m + rho c                             (K x T)
//   M_m = a^2 (H_m - rho H_m R H_m) + a rho (H_m R + R H_m) + rho^2 R H                        (K x K, symmetric)
// and for row j of shard m with loading row l_j:  yhat_j = l_j t_m,  cv_j = l_j (I - M_m) l_j' + omega_j.
// There is no branch on the mask after the Gram: the formulas hold on every row.
//
// Launch chain behind the sample save on the sweep stream (kernel boundaries order the stages):
//   1. k_precision (launch_precision_masked) at nv = T with Y* in V's place, the mask and the S^{-1} output: its
//      scratch then holds every [H_m | F_m] (term), [H | F] (rsum), X (xs), and the draw [q | ld];
//   2. k_predict_prod, a block per (16-column panel, shard): the K x K products R H_m, R H, H_m R, H_m (R H_m) and the
//      K x T ones H_m X, H X by mat_apply over LDS; k_predict_coef, a block per shard: t_m and N_m = I - M_m from
//      them, N_m stored symmetric bit for bit (the lower triangle computed and mirrored); block 0 also keeps
//      diag q and ld;
//   3. k_predict_apply, a block per 32 loading rows of a shard: the rows staged in LDS, [yhat | l N_m] =
//      l [t_m | N_m] on v_mfma_f64_16x16x4 (A = the rows from LDS, B = the coefficients from L2: at K = 128, T = 32
//      they are 164 KB, more than a CU's LDS), cv_j = (l_j N_m) . l_j + omega_j by a fixed-order row sum, and the
//      accumulators updated in place, each element owned by one thread.
// One sample is added per launch in sample order, no floating-point atomics, fixed summation orders and trip
// counts that depend on K and T only: the same inputs give the same bits however a run is cut into calls, and a
// NaN state runs through to NaN outputs.  Padding (rows j >= P of a shard, columns >= K or >= T) is never stored.
// One rank only: the close needs the global H and F at save time.
#include "handle.h"
#include "handoff.h"
#include "gj.h"

namespace dcfm {

constexpr int PRED_ROWS = 32;     // loading rows of a k_predict_apply block

// per-shard K x K / K x T work of k_predict_prod: H_m R, H_m R H_m, R H, R H_m, H_m X, H X
static size_t predict_work_doubles(int K, int T) { return 4 * (size_t)K * K + 2 * (size_t)K * T; }
static size_t predict_prod_lds(int K) { return ((size_t)K * K + (size_t)K * PREC_PANEL + 2) * sizeof(double); }
static size_t predict_apply_lds(int K) {
    const size_t K4 = (size_t)(K + 3) & ~(size_t)3, nkt = (size_t)(K + 15) / 16;
    return PRED_ROWS * ((K4 + 1) + (16 * nkt + 1)) * sizeof(double);
}

// A (K x K, LDS) = src (rows ld apart, global, agent-scope)
__device__ __forceinline__ void load_square(double *A, int K, const double *src, int ld) {
    for (int e = threadIdx.x; e < K * K; e += 256) {
        const int i = e / K, j = e - i * K;
        A[e] = ld_agent(src + (size_t)i * ld + j);
    }
}

// ---- 2a. the K x K and K x T products of shard m, one block per 16-column panel of the result (grid (panels, G)):
// panel c < nkt holds columns [16 c, 16 c + 16) of R H_m, R H, H_m R and H_m (R H_m); a panel behind them 16
// columns of H_m X and H X.  mat_apply forms every column on its own, so the split changes no bit of a product
__global__ __launch_bounds__(256) void k_predict_prod(const double *term, const double *rsum, const double *xs,
                                                      const double *sinv, int K, int T, double *work) {
    extern __shared__ __align__(16) double dyn[];
    double *A = dyn, *sP = dyn + K * K;
    const int m = blockIdx.y, w = K + T, nkt = (K + 15) / 16;
    const size_t ts = (size_t)K * w + (size_t)T * T + 1, KK = (size_t)K * K;
    const double *tm = term + (size_t)m * ts;
    double *wk = work + (size_t)m * (4 * KK + 2 * (size_t)K * T);
    double *HR = wk, *HRH = HR + KK, *RH = HRH + KK, *RHm = RH + KK, *HmX = RHm + KK, *HX = HmX + (size_t)K * T;
    if ((int)blockIdx.x < nkt) {
        const int c0 = PREC_PANEL * blockIdx.x, nc = min(PREC_PANEL, K - c0);
        load_square(A, K, sinv, K);                       // R
        mat_apply(A, K, tm + c0, w, nc, RHm + c0, K, sP);     // R H_m
        mat_apply(A, K, rsum + c0, w, nc, RH + c0, K, sP);    // R H
        stores_done();
        load_square(A, K, tm, w);                         // H_m
        mat_apply(A, K, sinv + c0, K, nc, HR + c0, K, sP);    // H_m R
        mat_apply(A, K, RHm + c0, K, nc, HRH + c0, K, sP);    // H_m (R H_m)
    } else {
        const int c0 = PREC_PANEL * ((int)blockIdx.x - nkt), nc = min(PREC_PANEL, T - c0);
        load_square(A, K, tm, w);                         // H_m
        mat_apply(A, K, xs + c0, T, nc, HmX + c0, T, sP);     // H_m X
        load_square(A, K, rsum, w);                       // H
        mat_apply(A, K, xs + c0, T, nc, HX + c0, T, sP);      // H X
    }
}

// ---- 2b. shard m's coefficients coef[m] = [t_m (K x Tp) | N_m (K x 16 nkt)], rows wc apart; the padding columns
// and rows stay the zeros they were allocated as.  Block 0 also keeps the sample's draw
__global__ __launch_bounds__(256) void k_predict_coef(const double *__restrict__ term, const double *__restrict__ rsum,
                                                      const double *__restrict__ qd, int K, int T, int Tp, int wc,
                                                      double rho, const double *__restrict__ work,
                                                      double *__restrict__ coef, double *__restrict__ draw) {
    const int m = blockIdx.x, t = threadIdx.x, w = K + T, K4 = (K + 3) & ~3;
    const size_t ts = (size_t)K * w + (size_t)T * T + 1, KK = (size_t)K * K;
    const double *tm = term + (size_t)m * ts;
    const double *wk = work + (size_t)m * (4 * KK + 2 * (size_t)K * T);
    const double *HR = wk, *HRH = HR + KK, *RH = HRH + KK, *HmX = RH + 2 * KK, *HX = HmX + (size_t)K * T;
    double *cm = coef + (size_t)m * K4 * wc;
    const double a = 1.0 - rho;
    for (int e = t; e < K * T; e += 256) {                // t_m = a (F_m - rho H_m X) + rho (F - rho H X)
        const int i = e / T, c = e - i * T;
        const double c_m = fma(-rho, HmX[e], tm[(size_t)i * w + K + c]);
        const double c_all = fma(-rho, HX[e], rsum[(size_t)i * w + K + c]);
        cm[(size_t)i * wc + c] = fma(a, c_m, rho * c_all);
    }
    for (int e = t; e < K * K; e += 256) {                // N_m = I - M_m: the lower triangle, mirrored
        const int i = e / K, j = e - i * K;
        if (i < j) continue;
        const double h = fma(-rho, HRH[e], tm[(size_t)i * w + j]);
        const double x = HR[e] + HR[(size_t)j * K + i];
        double mm = a * a * h;
        mm = fma(a * rho, x, mm);
        mm = fma(rho * rho, RH[e], mm);
        const double v = (i == j ? 1.0 : 0.0) - mm;
        cm[(size_t)i * wc + Tp + j] = v;
        cm[(size_t)j * wc + Tp + i] = v;
    }
    if (m == 0)                                           // the sample's draw [diag q | ld]
        for (int c = t; c <= T; c += 256) draw[c] = c < T ? qd[(size_t)c * T + c] : qd[(size_t)T * T];
}

// ---- 3. rows [32 b, 32 b + 32) of shard m: sum += yhat, sum2 += yhat^2 ([G P][T] row-major), cvsum += cv.
// Wave `wave` takes the 16 x 16 output tiles wave, wave + 4, .. of the 2 x (Tp / 16 + nkt) grid; a tile of the
// yhat columns goes straight to the accumulators from the MFMA C/D layout (row = q + 4 g, column = lane & 15: 128
// contiguous bytes per row), a tile of l N_m to LDS for the row sums.  grid (ceil(P / 32), G)
__global__ __launch_bounds__(256) void k_predict_apply(const double *__restrict__ Lam, const double *__restrict__ omega,
                                                       const double *__restrict__ coef, int P, int PP, int KW, int K,
                                                       int T, int Tp, int wc, double *__restrict__ sum,
                                                       double *__restrict__ sum2, double *__restrict__ cvsum) {
    extern __shared__ __align__(16) double dyn[];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, kq = lane >> 4;
    const int K4 = (K + 3) & ~3, ldl = K4 + 1, nkt = (K + 15) / 16, ldr = 16 * nkt + 1, nyt = Tp / 16;
    double *sL = dyn, *sR = dyn + PRED_ROWS * ldl;
    const int r0 = PRED_ROWS * blockIdx.x, m = blockIdx.y;
    const double *Lm = Lam + (size_t)m * PP * KW, *cm = coef + (size_t)m * K4 * wc;
    for (int e = t; e < PRED_ROWS * K4; e += 256) {
        const int r = e / K4, k = e - r * K4;
        sL[r * ldl + k] = (r0 + r < P && k < K) ? Lm[(size_t)(r0 + r) * KW + k] : 0.0;
    }
    __syncthreads();
    for (int item = wave; item < 2 * (nyt + nkt); item += 4) {
        const int rt = item & 1, ct = item >> 1;
        const double *ap = sL + (16 * rt + li) * ldl + kq;
        const double *bp = cm + (size_t)kq * wc + 16 * ct + li;
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < K4; k0 += 4) acc = mfma16x16x4(ap[k0], bp[(size_t)k0 * wc], acc);
        if (ct < nyt) {
            const int c = 16 * ct + li;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int j = r0 + 16 * rt + kq + 4 * g;
                if (j < P && c < T) {
                    const size_t idx = ((size_t)m * P + j) * T + c;
                    sum[idx] += acc[g];
                    sum2[idx] = fma(acc[g], acc[g], sum2[idx]);
                }
            }
        } else {
            const int k = 16 * (ct - nyt) + li;
#pragma unroll
            for (int g = 0; g < 4; ++g) sR[(16 * rt + kq + 4 * g) * ldr + k] = acc[g];
        }
    }
    __syncthreads();
    {   // cv of row r = t >> 3: eight threads' strided partial sums in k order, then a fixed tree
        const int r = t >> 3, part = t & 7;
        double s = 0.0;
        for (int k = part; k < K; k += 8) s = fma(sR[r * ldr + k], sL[r * ldl + k], s);
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        if (part == 0 && r0 + r < P) cvsum[(size_t)m * P + r0 + r] += s + omega[(size_t)m * PP + r0 + r];
    }
}

void launch_predict(const Dims &d, const Bufs &b, const Predict &pd, int64_t s, hipStream_t st) {
    launch_precision_masked(d, b, pd.pr, pd.obs, pd.sinv, pd.qd, st);
    hipLaunchKernelGGL(k_predict_prod, dim3(cdiv(d.K, PREC_PANEL) + pd.Tp / PREC_PANEL, d.G), dim3(256),
                       predict_prod_lds(d.K), st, pd.pr.term, pd.pr.rsum, pd.pr.xs, pd.sinv, d.K, pd.T, pd.work);
    hipLaunchKernelGGL(k_predict_coef, dim3(d.G), dim3(256), 0, st, pd.pr.term, pd.pr.rsum, pd.qd, d.K, pd.T, pd.Tp,
                       pd.wc, d.rho, pd.work, pd.coef, pd.draws + (size_t)s * (pd.T + 1));
    hipLaunchKernelGGL(k_predict_apply, dim3(cdiv(d.P, PRED_ROWS), d.G), dim3(256), predict_apply_lds(d.K), st, b.Lam,
                       b.omega, pd.coef, d.P, d.PP, d.kp, d.K, pd.T, pd.Tp, pd.wc, pd.sum, pd.sum2, pd.cvsum);
}

}  // namespace dcfm

extern "C" {

int dcfm_set_predict(dcfm_handle *h, const double *Ynew, const uint8_t *observed, int32_t nt, int64_t capacity) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    const Dims &d = h->d;
    if (capacity < 0) return fail(h, DCFM_ERR_INVALID, "set_predict: capacity %lld < 0", (long long)capacity);
    if (nt < 0 || nt > PROBE_NV_MAX)
        return fail(h, DCFM_ERR_INVALID, "set_predict: nt = %d outside 0..%d", (int)nt, PROBE_NV_MAX);
    if (capacity > 0) {
        if (!observed || (!Ynew && nt > 0)) return fail(h, DCFM_ERR_INVALID, "null argument");
        // Sigma_AA(s)'s closing step needs H and F summed over ALL shards on the device at save time: one more
        // all-gather per saved sample, which the sweep does not have
        if (d.coll)
            return fail(h, DCFM_ERR_UNSUPPORTED, "set_predict: conditional prediction needs the sum over all shards of "
                                                 "H_m and F_m on the device at every saved sample; a handle on the collective "
                                                 "path (nranks > 1 or COMM_SELF) has no such all-gather yet -- use one rank");
        for (size_t c = 0; c < (size_t)nt; ++c)
            for (size_t j = 0; j < (size_t)d.p; ++j)
                if (observed[j] && !std::isfinite(Ynew[c * d.p + j]))
                    return fail(h, DCFM_ERR_INVALID, "set_predict: observed Ynew(%zu, %zu) is not finite", j + 1, c + 1);
    }
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    Predict pd{};
    double *mem = nullptr;
    if (capacity > 0) {
        HIPC(h, precision_setup());
        HIPC(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_predict_prod), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)predict_prod_lds(KP_MAX)));
        HIPC(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_predict_apply), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)predict_apply_lds(KP_MAX)));
        const size_t T = (size_t)nt, K = (size_t)d.K, K4 = (K + 3) & ~(size_t)3, rows = (size_t)d.G * d.P;
        pd.T = nt;
        pd.Tp = (nt + 15) / 16 * 16;
        pd.wc = pd.Tp + (d.K + 15) / 16 * 16;
        const size_t nscr = precision_scratch_doubles(d, nt), nV = rows * T, nq = T * T + 1,
                     nwork = (size_t)d.G * predict_work_doubles(d.K, nt), ncoef = (size_t)d.G * K4 * pd.wc,
                     nacc = 2 * rows * T + rows, ndraw = (size_t)capacity * (T + 1), nobs = (rows + 7) / 8;
        void *q = nullptr;
        if (hipMalloc(&q, (nscr + nV + K * K + nq + nwork + ncoef + nacc + ndraw + nobs) * sizeof(double)) != hipSuccess)
            return fail(h, DCFM_ERR_ALLOC, "set_predict: %lld samples of %d new rows", (long long)capacity, (int)nt);
        mem = static_cast<double *>(q);
        precision_scratch_carve(d, nt, mem, pd.pr);
        double *dV = mem + nscr;
        pd.pr.V = dV;
        pd.sinv = dV + nV;
        pd.qd = pd.sinv + K * K;
        pd.work = pd.qd + nq;
        pd.coef = pd.work + nwork;
        pd.sum = pd.coef + ncoef;
        pd.sum2 = pd.sum + rows * T;
        pd.cvsum = pd.sum2 + rows * T;
        pd.draws = pd.cvsum + rows;
        pd.obs = reinterpret_cast<unsigned char *>(pd.draws + ndraw);
        // this rank's rows of Y*, row-major, the unobserved entries masked to zero here (never by a product: they
        // may be NaN), and the mask as 0 / 1 bytes
        std::vector<double> loc(nV);
        std::vector<unsigned char> ob(nobs * 8, 0);
        const size_t row0 = (size_t)d.shard0 * d.P;
        for (size_t j = 0; j < rows; ++j) {
            ob[j] = observed[row0 + j] ? 1 : 0;
            for (size_t c = 0; c < T; ++c) loc[j * T + c] = ob[j] ? Ynew[c * d.p + row0 + j] : 0.0;
        }
        hipError_t e = hipMemset(mem, 0, precision_ticket_doubles(d) * sizeof(double));   // tickets start at 0
        // the coefficients' padding and the accumulators start at 0
        if (e == hipSuccess) e = hipMemset(pd.coef, 0, (ncoef + nacc) * sizeof(double));
        if (e == hipSuccess && nV) e = hipMemcpy(dV, loc.data(), nV * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(pd.obs, ob.data(), nobs * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(mem);
            return fail(h, DCFM_ERR_HIP, "set_predict: %s", hipGetErrorString(e));
        }
    }
    if (h->pred_mem) (void)hipFree(h->pred_mem);
    h->pred_mem = mem;
    h->pred = pd;
    h->pred_cap = capacity;
    h->pred_n = 0;
    return DCFM_OK;
}

int dcfm_get_predict(dcfm_handle *h, double *mean, double *m2, double *cvar, double *maha, double *logdet,
                     int64_t *count) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    if (!count) return fail(h, DCFM_ERR_INVALID, "null argument");
    const Dims &d = h->d;
    const Predict &pd = h->pred;
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    const size_t S = (size_t)h->pred_n, T = (size_t)pd.T, rows = (size_t)d.G * d.P;
    *count = h->pred_n;
    if (S == 0 || !(mean || m2 || cvar || maha || logdet)) return DCFM_OK;
    const double cnt = (double)S;                         // the samples accumulated (the population form)
    std::vector<double> host(std::max(rows * std::max(T, (size_t)1), S * (T + 1)));
    for (int which = 0; which < 2; ++which) {
        double *out = which ? m2 : mean;
        if (!out || !T) continue;
        HIPC(h, hipMemcpy(host.data(), which ? pd.sum2 : pd.sum, rows * T * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t j = 0; j < rows; ++j)
            for (size_t c = 0; c < T; ++c) out[c * rows + j] = host[j * T + c] / cnt;
    }
    if (cvar) {
        HIPC(h, hipMemcpy(host.data(), pd.cvsum, rows * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t j = 0; j < rows; ++j) cvar[j] = host[j] / cnt;
    }
    if (maha || logdet) {
        HIPC(h, hipMemcpy(host.data(), pd.draws, S * (T + 1) * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < S; ++s) {
            if (maha) std::copy_n(host.data() + s * (T + 1), T, maha + s * T);
            if (logdet) logdet[s] = host[s * (T + 1) + T];
        }
    }
    return DCFM_OK;
}

}  // extern "C"
