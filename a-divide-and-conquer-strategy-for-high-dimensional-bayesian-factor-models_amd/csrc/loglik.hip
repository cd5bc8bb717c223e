// Pointwise log-likelihood of the training rows per saved sample (dcfm_set_loglik / dcfm_get_loglik):
//   l[s, i] = log N(y_i; 0, Sigma(s)) = -(p log 2 pi + log det Sigma(s) + y_i' Sigma(s)^{-1} y_i) / 2
// for every saved sample s and every row i of the standardised data the sweep holds, the input of WAIC
// (diagnostics.waic) and of PSIS-LOO.  The device records q_i = y_i' Sigma(s)^{-1} y_i and log det Sigma(s).
//
// The recursion is precision.hip's nested Woodbury with the n data rows as the probes, turned so that the
// only p-sized work is one more pass over Y.  With a = 1 - rho, Omega_m = diag(omega_m), per local shard m
//   T_m = Y_m Omega_m^{-1} Lambda_m  (n x K),   s_m[i] = sum_j Y_m[i, j]^2 / omega_mj,
//   G_m = Lambda_m' Omega_m^{-1} Lambda_m,  B_m = I + a G_m,  H_m = B_m^{-1} G_m,  ld_m = sum_j log omega_mj + log det B_m,
//   f_{m,i} = B_m^{-1} t_{m,i}
// and over the shards, S = I + rho sym(H):
//   u_i = sum_m f_{m,i},  H = sum_m H_m,  q_i = sum_m (s_m[i] - a t_{m,i}.f_{m,i}) - rho u_i' S^{-1} u_i,
//   log det Sigma(s) = sum_m ld_m + log det S.
// B_m and S keep the identity unscaled, so rho = 0 and rho = 1 need no special case.
//
// Launch chain behind the sample save on the sweep stream (kernel boundaries order the stages):
//   1. k_loglik_ypass<KW>  the Y pass, fp64 MFMA: wpass_acc's tiling, register ring and XCD remap with the
//      weight 1 / omega_j in place of omega_j, each lane also accumulating y^2 / omega_j of the Y elements it
//      has loaded; T_m -> T, s_m -> sq;
//   2. k_precision at nv = 0 (launch_precision_terms): the shards' G_m, B_m^{-1} (kept: binv), H_m, ld_m and the
//      rank's sum [H_r | ld_r] in its fixed shard and group orders;
//   3. k_loglik_sinv (one rank, one block): S^{-1} by gj_invert and log det Sigma(s);
//   4. k_loglik_shard, a block per (16 rows, shard): f = B_m^{-1} t and s - a t.f, in place over T_m and s_m;
//      k_loglik_close, 16 rows a block: u_i and the shards' terms summed in local shard order, then
//      q_i -= rho u_i' S^{-1} u_i and the draw [q (n) | ld]; several ranks store
//      [U_r (n x K) | q_r (n) | H_r | ld_r], which the read-out gathers in one collective over all draws, adds
//      in rank order and closes on the host with a K x K Cholesky, identically on every rank.
// No floating-point atomics, fixed summation orders, no data-dependent trip count: the same inputs give the
// same bits, and a NaN state runs through to NaN draws.  Rows i >= n of the padded layouts are computed by the
// pass (they are zeros of Y) and never stored into a draw.
//
// Operating point: stage 1 reads Y once (the bytes and MFMAs of k_wpass) plus one reciprocal per staged j and
// one FMA per loaded Y element; stages 2-4 are K x K or n x K: plain fp64 FMA over LDS operands (n K^2 g flops).
// DESIGN.md 4g has the measurements.
#include "handle.h"
#include "handoff.h"
#include "ypass.h"
#include "gj.h"

namespace dcfm {

constexpr int LL_ROWS = 16;       // rows of a k_loglik_close block

// ---- 1. the Y pass: acc as wpass_acc (lane (r, q) ends with T[i0 + 16a + r][32 kt + 8g + 2q + tb] in
// acc[a][tb][g]); ss[a] = this lane's share of s_m[i0 + 16a + r], the columns j = 8t + 2q, 8t + 2q + 1 of every
// chunk t in t order.  The weight 1 / omega_j is formed once per staged j by rcp_f64 (the hardware estimate and
// three correction terms: full fp64 precision for a fraction of the division's instructions -- the pass's VALU
// work does not overlap its MFMAs); a padding column j >= P of the last partial chunk takes weight 0 (Y is zero
// there, omega need not be invertible)
template <int KW, int MT, int R = (KW > KP ? WP_RING_WIDE : WP_RING)>
__device__ __forceinline__ void tpass_acc(const Dims &d, const double *__restrict__ Y, const double *__restrict__ Lam,
                                          const double *__restrict__ omega, int m, int i0, int kt, d4 (&acc)[MT][2],
                                          double (&ss)[MT]) {
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const double *Y0 = Y + ((size_t)m * d.NP + i0 + r) * d.PP + 2 * q;
    const double *Y1 = Y0 + (size_t)16 * (MT - 1) * d.PP;
    const double *L = Lam + (size_t)m * d.PP * KW + 32 * kt + 2 * r;
    const double *wp = omega + (size_t)m * d.PP + 2 * q;
    d4 acc2[MT][2];
#pragma unroll
    for (int a = 0; a < MT; ++a) {
        ss[a] = 0.0;
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = acc2[a][b] = d4{0.0, 0.0, 0.0, 0.0};
    }
    const int nch = (d.P + 7) >> 3;                       // as wpass_acc: whole padding chunks hold zeros of Y
    d2 y0[R], y1[R], ww[R], l0[R], l1[R];
    auto load = [&](int t, int k) {
        const int j = 8 * t;
        y0[k] = *reinterpret_cast<const d2 *>(Y0 + j);
        if (MT == 2) y1[k] = *reinterpret_cast<const d2 *>(Y1 + j);
        ww[k] = *reinterpret_cast<const d2 *>(wp + j);
        l0[k] = *reinterpret_cast<const d2 *>(L + (size_t)(j + 2 * q) * KW);
        l1[k] = *reinterpret_cast<const d2 *>(L + (size_t)(j + 2 * q + 1) * KW);
    };
    auto mma = [&](int t, int k) {
        const int j = 8 * t + 2 * q;
        const double w0 = j < d.P ? rcp_f64(ww[k].x) : 0.0, w1 = j + 1 < d.P ? rcp_f64(ww[k].y) : 0.0;
        const double b00 = w0 * l0[k].x, b01 = w0 * l0[k].y;
        const double b10 = w1 * l1[k].x, b11 = w1 * l1[k].y;
        acc[0][0] = mfma16x16x4(b00, y0[k].x, acc[0][0]);
        acc[0][1] = mfma16x16x4(b01, y0[k].x, acc[0][1]);
        if (MT == 2) {
            acc[MT - 1][0] = mfma16x16x4(b00, y1[k].x, acc[MT - 1][0]);
            acc[MT - 1][1] = mfma16x16x4(b01, y1[k].x, acc[MT - 1][1]);
        }
        acc2[0][0] = mfma16x16x4(b10, y0[k].y, acc2[0][0]);
        acc2[0][1] = mfma16x16x4(b11, y0[k].y, acc2[0][1]);
        if (MT == 2) {
            acc2[MT - 1][0] = mfma16x16x4(b10, y1[k].y, acc2[MT - 1][0]);
            acc2[MT - 1][1] = mfma16x16x4(b11, y1[k].y, acc2[MT - 1][1]);
        }
        ss[0] = fma(y0[k].x * y0[k].x, w0, ss[0]);
        ss[0] = fma(y0[k].y * y0[k].y, w1, ss[0]);
        if (MT == 2) {
            ss[MT - 1] = fma(y1[k].x * y1[k].x, w0, ss[MT - 1]);
            ss[MT - 1] = fma(y1[k].y * y1[k].y, w1, ss[MT - 1]);
        }
    };
#pragma unroll
    for (int k = 0; k < R - 1; ++k)
        if (k < nch) load(k, k);
    for (int t = 0; t < nch; t += R) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (t + k + R - 1 < nch) load(t + k + R - 1, (k + R - 1) % R);
            if (t + k < nch) mma(t + k, k);
        }
    }
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] += acc2[a][b];
}

// 1-D grid as k_wpass: (shard, 128-row block) x the KW / 32 column tiles, adjacent (same XCD: Y from L2)
template <int KW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KW == KP ? 3 : 2))) void k_loglik_ypass(Dims d, const double *__restrict__ Y, const double *__restrict__ Lam,
                                                      const double *__restrict__ omega, double *__restrict__ T,
                                                      double *__restrict__ sq) {
    constexpr int MT = 2;
    const int w = xcd_remap(blockIdx.x, gridDim.x), wt = w / (KW / 32), kt = w % (KW / 32);
    const int nrb = d.NP / (64 * MT), m = wt / nrb, rb = wt % nrb;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int i0 = rb * 64 * MT + wave * 16 * MT;
    d4 acc[MT][2];
    double ss[MT];
    tpass_acc<KW, MT>(d, Y, Lam, omega, m, i0, kt, acc, ss);
#pragma unroll
    for (int a = 0; a < MT; ++a) {
        double *Tt = T + ((size_t)m * d.NP + i0 + 16 * a + r) * KW + 32 * kt + 2 * q;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            d2 v;
            v.x = acc[a][0][g];
            v.y = acc[a][1][g];
            *reinterpret_cast<d2 *>(Tt + 8 * g) = v;
        }
        // the row's four lanes q: (q0 + q1) + (q2 + q3), the same value in each
        double s = ss[a];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (kt == 0 && q == 0) sq[(size_t)m * d.NP + i0 + 16 * a + r] = s;
    }
}

// ---- 3. one rank: sinv = [S^{-1} (K x K) | log det Sigma(s)], S = I + rho sym(H) from hsum = [H | sum ld_m]
__global__ __launch_bounds__(256) void k_loglik_sinv(const double *__restrict__ hsum, int K, double rho,
                                                     double *__restrict__ sinv) {
    extern __shared__ __align__(16) double dyn[];
    double *A = dyn, *Cc = dyn + K * K + (K & 1);         // Cc: 16-byte aligned
    const int t = threadIdx.x;
    for (int e = t; e < K * K; e += 256) {
        const int i = e / K, j = e - i * K;
        A[e] = fma(rho, 0.5 * (hsum[e] + hsum[j * K + i]), i == j ? 1.0 : 0.0);
    }
    const double ldS = gj_invert(A, K, Cc);
    for (int e = t; e < K * K; e += 256) sinv[e] = A[e];
    if (t == 0) sinv[K * K] = hsum[K * K] + ldS;
}

// f = M x for the block's LL_ROWS rows: M (K x K) in sM with rows ldm apart, x in sX with rows ldm apart; thread
// (row = t & 15, kg = t >> 4) forms f[u] = f_{kg + 16 u}, u < LL_NU = KW / 16 (zero for an index >= K), and the
// rows' x.f lands in dot[row] as the sum over kg in kg order of each thread's sum over u in u order
template <int LL_NU>
__device__ __forceinline__ void rows_apply(const double *sM, const double *sX, int K, int ldm, double (&f)[LL_NU],
                                           double *red, double *dot) {
    const int t = threadIdx.x, row = t & 15, kg = t >> 4;
    const double *x = sX + row * ldm;
    int ro[LL_NU];
#pragma unroll
    for (int u = 0; u < LL_NU; ++u) {
        f[u] = 0.0;
        ro[u] = min(kg + 16 * u, K - 1) * ldm;
    }
#pragma unroll 2
    for (int j = 0; j < K; ++j) {
        const double b = x[j];
#pragma unroll
        for (int u = 0; u < LL_NU; ++u) f[u] = fma(sM[ro[u] + j], b, f[u]);
    }
    double part = 0.0;
#pragma unroll
    for (int u = 0; u < LL_NU; ++u) {
        const int k = kg + 16 * u;
        if (k >= K) f[u] = 0.0;
        part = fma(x[min(k, K - 1)], f[u], part);
    }
    red[row * 16 + kg] = part;
    __syncthreads();
    if (t < LL_ROWS) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 16; ++c) s += red[t * 16 + c];
        dot[t] = s;
    }
    __syncthreads();
}

// ---- 4a. shard m's term of rows [16 b, 16 b + 16), in place: T_m's rows become F_m's (f = B_m^{-1} t) and
// sq_m[i] becomes s_m[i] - (1 - rho) t_i.f_i.  A block reads its rows into LDS before it overwrites them and no
// other block touches them.  grid (row blocks, G)
template <int LL_NU>
__global__ __launch_bounds__(256) void k_loglik_shard(double *__restrict__ T, double *__restrict__ sq,
                                                      const double *__restrict__ binv, int NP, int KW, int K, double rho) {
    extern __shared__ __align__(16) double dyn[];
    const int ldm = K | 1;                                // odd: the 16 rows' x[j] on distinct banks
    double *sM = dyn, *sX = sM + K * ldm, *red = sX + LL_ROWS * ldm, *dot = red + LL_ROWS * 16;
    const int t = threadIdx.x, row = t & 15, kg = t >> 4, i0 = LL_ROWS * blockIdx.x, m = blockIdx.y;
    for (int e = t; e < K * K; e += 256) sM[(e / K) * ldm + e % K] = binv[(size_t)m * K * K + e];
    for (int e = t; e < LL_ROWS * K; e += 256) {          // i0 + 15 < NP: NP is a multiple of 16
        const int rr = e / K, k = e - rr * K;
        sX[rr * ldm + k] = T[((size_t)m * NP + i0 + rr) * KW + k];
    }
    __syncthreads();
    double f[LL_NU];
    rows_apply(sM, sX, K, ldm, f, red, dot);
    double *Fr = T + ((size_t)m * NP + i0 + row) * KW;
#pragma unroll
    for (int c = 0; c < LL_NU; ++c)
        if (kg + 16 * c < K) Fr[kg + 16 * c] = f[c];
    if (kg == 0) {
        double *sp = sq + (size_t)m * NP + i0 + row;
        *sp = fma(-(1.0 - rho), dot[row], *sp);
    }
}

// ---- 4b. the close of rows [16 b, 16 b + 16): u_i = sum_m f_{m,i} and q_i = sum_m of the shards' terms, both from
// 0 in local shard order (sixteen loads in flight per thread), then q_i -= rho u_i' S^{-1} u_i.  form: one rank,
// out = [q (n) | ld]; else the rank's partial out = [U_r (n x K, row-major) | q_r (n) | H_r (K x K) | ld_r]
template <int LL_NU>
__global__ __launch_bounds__(256) void k_loglik_close(const double *__restrict__ F, const double *__restrict__ sq,
                                                      const double *__restrict__ hsum, const double *__restrict__ sinv,
                                                      int n, int NP, int KW, int K, int G, double rho, int form,
                                                      double *__restrict__ out) {
    extern __shared__ __align__(16) double dyn[];
    constexpr int FK = 16;
    const int ldm = K | 1;
    double *sM = dyn, *sX = sM + K * ldm, *red = sX + LL_ROWS * ldm, *dot = red + LL_ROWS * 16;
    const int t = threadIdx.x, i0 = LL_ROWS * blockIdx.x;
    const size_t ms = (size_t)NP * KW;                    // a shard's stride in F
    double *U = out, *qr = out + (size_t)n * K, *Hr = qr + n;
    {   // thread (rr = t >> 4, kl = t & 15): u of row i0 + rr, columns kl + 16 c -- 128 contiguous bytes a row
        const int rr = t >> 4, kl = t & 15;
        for (int c = 0; c < LL_NU; ++c) {
            const int k = kl + 16 * c;
            if (k >= K) break;
            const double *src = F + (size_t)(i0 + rr) * KW + k;
            double acc = 0.0;
            for (int m0 = 0; m0 < G; m0 += FK) {
                double v[FK];
#pragma unroll
                for (int j = 0; j < FK; ++j) v[j] = src[(size_t)min(m0 + j, G - 1) * ms];
#pragma unroll
                for (int j = 0; j < FK; ++j)
                    if (m0 + j < G) acc += v[j];
            }
            if (form) sX[rr * ldm + k] = acc;
            else if (i0 + rr < n) U[(size_t)(i0 + rr) * K + k] = acc;
        }
    }
    double qi = 0.0;                                      // thread t < 16: row i0 + t (rows_apply's row of kg = 0)
    if (t < LL_ROWS)
        for (int m0 = 0; m0 < G; m0 += FK) {
            double v[FK];
#pragma unroll
            for (int j = 0; j < FK; ++j) v[j] = sq[(size_t)min(m0 + j, G - 1) * NP + i0 + t];
#pragma unroll
            for (int j = 0; j < FK; ++j)
                if (m0 + j < G) qi += v[j];
        }
    if (!form) {
        if (t < LL_ROWS && i0 + t < n) qr[i0 + t] = qi;
        if (blockIdx.x == 0)
            for (int e = t; e < K * K + 1; e += 256) Hr[e] = hsum[e];
        return;
    }
    for (int e = t; e < K * K; e += 256) sM[(e / K) * ldm + e % K] = sinv[e];
    __syncthreads();
    double f[LL_NU];
    rows_apply(sM, sX, K, ldm, f, red, dot);
    if (t < LL_ROWS && i0 + t < n) out[i0 + t] = fma(-rho, dot[t], qi);
    if (blockIdx.x == 0 && t == 0) out[n] = sinv[K * K];
}

static size_t loglik_close_lds(int K) {
    const size_t ldm = (size_t)(K | 1);
    return ((size_t)K * ldm + LL_ROWS * ldm + LL_ROWS * 16 + LL_ROWS) * sizeof(double);
}
static size_t loglik_sinv_lds(int K) { return ((size_t)K * K + (K & 1) + (size_t)K * GJ_B) * sizeof(double); }

void launch_loglik(const Dims &d, const Bufs &b, const LogLik &ll, int64_t s, hipStream_t st) {
    const dim3 grid((d.NP / 128) * d.G * (d.kp / 32));
    switch (d.kp) {
    case 32: hipLaunchKernelGGL(k_loglik_ypass<32>, grid, dim3(256), 0, st, d, b.Y, b.Lam, b.omega, ll.T, ll.sq); break;
    case 64: hipLaunchKernelGGL(k_loglik_ypass<64>, grid, dim3(256), 0, st, d, b.Y, b.Lam, b.omega, ll.T, ll.sq); break;
    default: hipLaunchKernelGGL(k_loglik_ypass<128>, grid, dim3(256), 0, st, d, b.Y, b.Lam, b.omega, ll.T, ll.sq); break;
    }
    launch_precision_terms(d, b, ll.pr, ll.binv, ll.hsum, st);
    const int form = d.coll ? 0 : 1;
    if (form) hipLaunchKernelGGL(k_loglik_sinv, dim3(1), dim3(256), loglik_sinv_lds(d.K), st, ll.hsum, d.K, d.rho, ll.sinv);
    const int nrb = (d.n + LL_ROWS - 1) / LL_ROWS;
    double *draw = ll.draws + (size_t)s * ll.slot;
#define DCFM_LL_CLOSE(NU)                                                                                              \
    hipLaunchKernelGGL(k_loglik_shard<NU>, dim3(nrb, d.G), dim3(256), ll.lds, st, ll.T, ll.sq, ll.binv, d.NP, d.kp, d.K, \
                       d.rho);                                                                                         \
    hipLaunchKernelGGL(k_loglik_close<NU>, dim3(nrb), dim3(256), ll.lds, st, ll.T, ll.sq, ll.hsum, ll.sinv, d.n, d.NP,  \
                       d.kp, d.K, d.G, d.rho, form, draw)
    switch (d.kp) {
    case 32: DCFM_LL_CLOSE(2); break;
    case 64: DCFM_LL_CLOSE(4); break;
    default: DCFM_LL_CLOSE(8); break;
    }
#undef DCFM_LL_CLOSE
}

}  // namespace dcfm

// Host close of the several-rank read-out: t = [U (n x K) | q (n) | H (K x K) | ld] summed over the ranks;
// S = I + rho sym(H) = R R' (plain Cholesky), z_i = R^{-1} u_i, maha[i] = q_i - rho z_i.z_i, returns
// ld + 2 sum log diag R.  Fixed trip counts: a NaN runs through
static double host_close_rows(const double *t, int n, int K, double rho, double *maha) {
    const double *U = t, *q = t + (size_t)n * K, *H = q + n;
    std::vector<double> R((size_t)K * K), z(K);
    double ld = H[(size_t)K * K];
    for (int j = 0; j < K; ++j) {
        for (int i = j; i < K; ++i) {
            double s = std::fma(rho, 0.5 * (H[(size_t)i * K + j] + H[(size_t)j * K + i]), i == j ? 1.0 : 0.0);
            for (int k = 0; k < j; ++k) s = std::fma(-R[(size_t)i * K + k], R[(size_t)j * K + k], s);
            R[(size_t)i * K + j] = i == j ? std::sqrt(s) : s / R[(size_t)j * K + j];
        }
        ld += 2.0 * std::log(R[(size_t)j * K + j]);
    }
    for (int r = 0; r < n; ++r) {
        double acc = 0.0;
        for (int i = 0; i < K; ++i) {
            double s = U[(size_t)r * K + i];
            for (int k = 0; k < i; ++k) s = std::fma(-R[(size_t)i * K + k], z[k], s);
            z[i] = s / R[(size_t)i * K + i];
            acc = std::fma(z[i], z[i], acc);
        }
        maha[r] = std::fma(-rho, acc, q[r]);
    }
    return ld;
}

extern "C" {

int dcfm_set_loglik(dcfm_handle *h, int64_t capacity) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    const Dims &d = h->d;
    if (capacity < 0) return fail(h, DCFM_ERR_INVALID, "set_loglik: capacity %lld < 0", (long long)capacity);
    // with a mask the rows the pass reads are completed by the current draw: that is the completed-data likelihood
    if (capacity > 0 && h->imp.nmiss)
        return fail(h, DCFM_ERR_UNSUPPORTED, "set_loglik: the handle has missing data (dcfm_set_missing); the rows' "
                                             "likelihood would be that of the completed data, not of the observed entries");
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    LogLik ll{};
    double *mem = nullptr;
    if (capacity > 0) {
        HIPC(h, precision_setup());
        // k_loglik_shard, k_loglik_close (147 KiB) and k_loglik_sinv (132 KiB) at K = 128 pass the default limit of dynamic LDS;
        // the attribute belongs to the kernel, so it is set to that whatever this handle's K
        for (const void *k : {reinterpret_cast<const void *>(k_loglik_shard<2>), reinterpret_cast<const void *>(k_loglik_shard<4>),
                              reinterpret_cast<const void *>(k_loglik_shard<8>), reinterpret_cast<const void *>(k_loglik_close<2>),
                              reinterpret_cast<const void *>(k_loglik_close<4>), reinterpret_cast<const void *>(k_loglik_close<8>)})
            HIPC(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)loglik_close_lds(KP_MAX)));
        HIPC(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_loglik_sinv), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)loglik_sinv_lds(KP_MAX)));
        const size_t n = (size_t)d.n, K = (size_t)d.K, nscr = precision_scratch_doubles(d, 0),
                     nT = (size_t)d.G * d.NP * d.kp, nsq = (size_t)d.G * d.NP, nb = (size_t)d.G * K * K, nh = K * K + 1;
        ll.slot = d.coll ? n * K + n + nh : n + 1;
        ll.lds = loglik_close_lds(d.K);
        void *q = nullptr;
        if (hipMalloc(&q, (nscr + nT + nsq + nb + 2 * nh + (size_t)capacity * ll.slot) * sizeof(double)) != hipSuccess)
            return fail(h, DCFM_ERR_ALLOC, "set_loglik: %lld draws of %d rows", (long long)capacity, d.n);
        mem = static_cast<double *>(q);
        precision_scratch_carve(d, 0, mem, ll.pr);
        ll.T = mem + nscr;
        ll.sq = ll.T + nT;
        ll.binv = ll.sq + nsq;
        ll.hsum = ll.binv + nb;
        ll.sinv = ll.hsum + nh;
        ll.draws = ll.sinv + nh;
        if (hipMemset(mem, 0, precision_ticket_doubles(d) * sizeof(double)) != hipSuccess) {   // tickets start at 0
            (void)hipFree(mem);
            return fail(h, DCFM_ERR_HIP, "set_loglik: hipMemset failed");
        }
    }
    if (h->ll_mem) (void)hipFree(h->ll_mem);
    h->ll_mem = mem;
    h->ll = ll;
    h->ll_cap = capacity;
    h->ll_n = 0;
    return DCFM_OK;
}

int dcfm_get_loglik(dcfm_handle *h, double *maha, double *logdet, int64_t *count) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    const Dims &d = h->d;
    const LogLik &ll = h->ll;
    int code = count ? DCFM_OK : fail(h, DCFM_ERR_INVALID, "null argument");
    if (code == DCFM_OK) {
        hipError_t e = hipSetDevice(h->cfg.device);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) code = fail(h, DCFM_ERR_HIP, "get_loglik: %s", hipGetErrorString(e));
    }
    const size_t S = (size_t)h->ll_n, n = (size_t)d.n, mine = S * ll.slot;
    const bool want = maha || logdet;
    if (!d.coll || S == 0) {   // one rank: the kernel closed the draw.  No draw (on every rank): nothing to gather
        if (code != DCFM_OK) return code;
        *count = h->ll_n;
        if (want && S) {
            std::vector<double> host(mine);
            HIPC(h, hipMemcpy(host.data(), ll.draws, mine * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t s = 0; s < S; ++s) {
                if (maha) std::copy_n(host.data() + s * ll.slot, n, maha + s * n);
                if (logdet) logdet[s] = host[s * ll.slot + n];
            }
        }
        return DCFM_OK;
    }
    // several ranks: every rank's [U_r | q_r | H_r | ld_r] of all draws in one all-gather, summed in rank order
    TRY(agree(h, code));
    *count = h->ll_n;
    const size_t nr = (size_t)d.nranks;
    void *g = nullptr;
    if (hipMalloc(&g, nr * mine * sizeof(double)) != hipSuccess)
        code = fail(h, DCFM_ERR_ALLOC, "get_loglik: gather of %zu doubles", nr * mine);
    if (int rc = agree(h, code)) {
        if (g) (void)hipFree(g);
        return rc;
    }
    double *all = static_cast<double *>(g);
    std::vector<double> host(want ? nr * mine : 0);
    int rc = coll_allgather(h, CH_MAIN, ll.draws, all, mine, h->stream);
    if (rc == DCFM_OK && want) {
        const hipError_t e = hipMemcpyAsync(host.data(), all, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) rc = fail(h, DCFM_ERR_HIP, "get_loglik: %s", hipGetErrorString(e));
    }
    const hipError_t es = hipStreamSynchronize(h->stream);
    (void)hipFree(all);
    if (rc == DCFM_OK && es != hipSuccess) rc = fail(h, DCFM_ERR_HIP, "get_loglik: %s", hipGetErrorString(es));
    if (rc != DCFM_OK || !want) return rc;
    std::vector<double> sum(ll.slot), q(n);
    for (size_t s = 0; s < S; ++s) {
        std::fill(sum.begin(), sum.end(), 0.0);
        for (size_t r = 0; r < nr; ++r) {
            const double *t = host.data() + (r * S + s) * ll.slot;
            for (size_t e = 0; e < ll.slot; ++e) sum[e] += t[e];
        }
        const double ld = host_close_rows(sum.data(), d.n, d.K, d.rho, q.data());
        if (maha) std::copy(q.begin(), q.end(), maha + s * n);
        if (logdet) logdet[s] = ld;
    }
    return DCFM_OK;
}

}  // extern "C"
