// Per-sample posterior draws of V' Sigma(s) V for a caller-chosen block of probe vectors
// (dcfm_set_probes / dcfm_get_probe_draws).
//
// The reference keeps only the running mean of Sigma (dc:180-196): the per-sample matrix exists for the
// instant in which the sample's Lambda and omega go into the assembly batch (k_lambda itself, K <= 32; else
// k_save).  Any functional of Sigma that
// is not one entry -- a portfolio variance v' Sigma v, a correlation, a ratio of variances, a credible
// interval -- needs its value per saved sample, and none needs Sigma(s) formed.  With L_m the P x K
// loadings of shard m, V_m the rows of V of that shard and W_m = L_m' V_m (K x nv), W = sum_m W_m,
//   Sigma(s)     = rho L L' + (1 - rho) blockdiag(L_m L_m') + diag(omega)                     (dc:182-192)
//   V' Sigma(s) V = rho W' W + sum_m [ (1 - rho) W_m' W_m + V_m' diag(omega_m) V_m ]
// k_probes runs behind the sample save on the sweep stream: slices x G blocks (probe_slices), each reducing a
// fixed slice of a shard's loading rows into a partial [W (K x nv) | V' Omega V (nv x nv)]; the last
// slice block of a shard (handoff.h's ticket) adds the slices in slice order and forms the shard's
// term [W_m | D_m = (1 - rho) W_m' W_m + V_m' Omega_m V_m]; the last shard block of a group of PROBE_FAN
// shards adds its shards' terms in shard order, and the last group block the groups' in group order (two
// levels: one block adding c3's 64 terms reads 0.76 MB alone) and writes the draw: one rank
// rho W' W + D itself, several ranks their [W_r | D_r], which the read-out gathers in one collective
// over all draws and sums in rank order.  No floating-point atomics and fixed orders throughout: the
// same inputs give the same bits.
//
// Operating point: plain fp64 FMA.  A draw is 2 p K nv flops (40 MFLOP at c3, 64 at c4 with nv = 32)
// over one read of Lambda and V (5-13 MB), spread over ~256 blocks that each stream a few tens of rows
// through LDS: measured the launch runs far below both the fp64 and the HBM rate, so it is
// bound by the latency of its four dependent steps (slice partials, then the shard, group and rank folds
// through L2), not by arithmetic.  fp64 MFMA (16x16x4) would shorten only the first and needs nv padded
// to 16 and Lambda' V fragments transposed through LDS for it.
#include "handle.h"
#include "handoff.h"

namespace dcfm {

constexpr int PROBE_ROWS = 32;    // loading rows staged per step
static_assert(PROBE_NV_MAX == 32, "k_probes maps a thread to column t & 31 and stages V rows 32 wide");

// element e of a [W | D] term is live: every W entry, and the lower triangle of D
__device__ __forceinline__ bool probe_live(int e, int nw, int nv) {
    return e < nw || (e - nw) / nv >= (e - nw) % nv;
}

// sL (W part) and sV (D part) = the sum of `count` terms, src[k * ts + e] over k in k order, for a term's live
// elements e.  The loads are agent-scope (handoff.h) and independent of one another: FE x FK of them are
// in flight per thread before the first is added (issued one at a time, 500-600 dependent L2 round trips
// per thread made the launch 195 us at c3); a load past the count or for a dead element
// re-reads a valid address and is dropped
__device__ __forceinline__ void fold_terms(const double *src, int count, int nw, int nv, double *sL, double *sV) {
    constexpr int FE = 4, FK = 8;
    const int ts = nw + nv * nv;
    for (int e0 = threadIdx.x; e0 < ts; e0 += 256 * FE) {
        int e[FE];
        bool on[FE];
        double acc[FE];
#pragma unroll
        for (int i = 0; i < FE; ++i) {
            e[i] = e0 + 256 * i;
            on[i] = e[i] < ts && probe_live(e[i], nw, nv);
            if (!on[i]) e[i] = 0;
            acc[i] = 0.0;
        }
        for (int k0 = 0; k0 < count; k0 += FK) {
            double v[FE][FK];
#pragma unroll
            for (int u = 0; u < FK; ++u)
#pragma unroll
                for (int i = 0; i < FE; ++i) v[i][u] = ld_agent(src + (size_t)min(k0 + u, count - 1) * ts + e[i]);
#pragma unroll
            for (int u = 0; u < FK; ++u)
#pragma unroll
                for (int i = 0; i < FE; ++i)
                    if (k0 + u < count) acc[i] += v[i][u];
        }
#pragma unroll
        for (int i = 0; i < FE; ++i)
            if (on[i]) (e[i] < nw ? sL[e[i]] : sV[e[i] - nw]) = acc[i];
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_probes(const double *__restrict__ Lam, const double *__restrict__ omega,
                                                const double *__restrict__ V, int P, int PP, int KW, int K, int G,
                                                int nv, double rho, int form, double *part, double *term,
                                                double *gterm, unsigned *ticket, double *__restrict__ draw) {
    // [rows of Lambda | rows of V | omega] of a step; then W_m (W_r) and V' Omega V of the folds
    __shared__ double sL[PROBE_ROWS * KP_MAX], sV[PROBE_ROWS * PROBE_NV_MAX], sO[PROBE_ROWS];
    __shared__ unsigned flag;
    const int sl = blockIdx.x, S = gridDim.x, m = blockIdx.y, t = threadIdx.x;
    const int c = t & 31, kg = t >> 5;                  // column of V; W rows kg + 8 i, D rows kg + 8 i
    const int nw = K * nv, ts = nw + nv * nv;           // doubles of a term
    const int j0 = (int)((long long)P * sl / S), j1 = (int)((long long)P * (sl + 1) / S);
    const double *Lm = Lam + (size_t)m * PP * KW, *Vm = V + (size_t)m * P * nv, *om = omega + (size_t)m * PP;
    // W rows and D rows per thread: wave-uniform counts, no per-lane test in the row loop (sL's padding
    // columns k >= K hold zeros, sV's columns c >= nv are staged as zeros)
    const int nI = KW / 8, nD = (nv + 7) / 8;
    double aw[KP_MAX / 8], ad[PROBE_NV_MAX / 8];
#pragma unroll
    for (int i = 0; i < KP_MAX / 8; ++i) aw[i] = 0.0;
#pragma unroll
    for (int i = 0; i < PROBE_NV_MAX / 8; ++i) ad[i] = 0.0;
    for (int r0 = j0; r0 < j1; r0 += PROBE_ROWS) {
        const int nr = min(PROBE_ROWS, j1 - r0);
        for (int e = t; e < nr * KW; e += 256) sL[e] = Lm[(size_t)r0 * KW + e];
        for (int e = t; e < nr * PROBE_NV_MAX; e += 256)
            sV[e] = (e & 31) < nv ? Vm[(size_t)(r0 + (e >> 5)) * nv + (e & 31)] : 0.0;
        if (t < nr) sO[t] = om[r0 + t];
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const double v = sV[r * PROBE_NV_MAX + c], w = sO[r];
#pragma unroll
            for (int i = 0; i < KP_MAX / 8; ++i)
                if (i < nI) aw[i] = fma(sL[r * KW + kg + 8 * i], v, aw[i]);
            // omega (V_a V_b): the product commutes, so the square is symmetric bit for bit
#pragma unroll
            for (int i = 0; i < PROBE_NV_MAX / 8; ++i)
                if (i < nD) ad[i] = fma(w, sV[r * PROBE_NV_MAX + kg + 8 * i] * v, ad[i]);
        }
        __syncthreads();
    }
    double *mine = part + ((size_t)m * S + sl) * ts;
    if (c < nv) {
#pragma unroll
        for (int i = 0; i < KP_MAX / 8; ++i)
            if (kg + 8 * i < K) st_agent(mine + (kg + 8 * i) * nv + c, aw[i]);
#pragma unroll
        for (int i = 0; i < PROBE_NV_MAX / 8; ++i)
            if (kg + 8 * i < nv) st_agent(mine + nw + (kg + 8 * i) * nv + c, ad[i]);
    }
    // the shard's last slice block: the slices in slice order, then the shard's term
    if (!last_arrival(ticket + m, S, &flag)) return;
    fold_terms(part + (size_t)m * S * ts, S, nw, nv, sL, sV);
    double *tm = term + (size_t)m * ts;
    for (int e = t; e < ts; e += 256) {
        if (!probe_live(e, nw, nv)) continue;
        double v = sL[e < nw ? e : 0];
        if (e >= nw) {
            const int a = (e - nw) / nv, b = (e - nw) % nv;
            double acc = 0.0;
            for (int k = 0; k < K; ++k) acc = fma(sL[k * nv + a], sL[k * nv + b], acc);
            v = fma(1.0 - rho, acc, sV[e - nw]);
        }
        st_agent(tm + e, v);
    }
    // the last shard block of a group of PROBE_FAN shards: its shards in shard order
    const int gi = m / PROBE_FAN, ng = (G + PROBE_FAN - 1) / PROBE_FAN;
    if (!last_arrival(ticket + G + gi, min(PROBE_FAN, G - gi * PROBE_FAN), &flag)) return;
    fold_terms(term + (size_t)gi * PROBE_FAN * ts, min(PROBE_FAN, G - gi * PROBE_FAN), nw, nv, sL, sV);
    for (int e = t; e < ts; e += 256)
        if (probe_live(e, nw, nv)) st_agent(gterm + (size_t)gi * ts + e, e < nw ? sL[e] : sV[e - nw]);
    // the rank's last group block: the groups in group order into the draw
    if (!last_arrival(ticket + G + ng, ng, &flag)) return;
    fold_terms(gterm, ng, nw, nv, sL, sV);
    if (!form)                                           // several ranks: W_r for the read-out's sum over ranks
        for (int e = t; e < nw; e += 256) draw[e] = sL[e];
    double *Q = form ? draw : draw + nw;
    for (int e = t; e < nv * nv; e += 256) {             // one triangle, mirrored
        const int a = e / nv, b = e % nv;
        if (a < b) continue;
        double v = sV[e];
        if (form) {
            double acc = 0.0;
            for (int k = 0; k < K; ++k) acc = fma(sL[k * nv + a], sL[k * nv + b], acc);
            v = fma(rho, acc, v);
        }
        Q[a * nv + b] = v;
        Q[b * nv + a] = v;
    }
}

void launch_probes(const Dims &d, const Bufs &b, const Probes &pr, int64_t s, hipStream_t st) {
    hipLaunchKernelGGL(k_probes, dim3(pr.slices, d.G), dim3(256), 0, st, b.Lam, b.omega, pr.V, d.P, d.PP, d.kp, d.K,
                       d.G, pr.nv, d.rho, d.coll ? 0 : 1, pr.part, pr.term, pr.gterm, pr.ticket, pr.draws + (size_t)s * pr.slot);
}

}  // namespace dcfm

// doubles of the tickets in front of the fold scratch: G shards, their groups, the rank
static int probe_groups(int G) { return (G + PROBE_FAN - 1) / PROBE_FAN; }
static size_t probe_ticket_doubles(int G) { return ((size_t)G + probe_groups(G) + 1 + 1) / 2; }

extern "C" {

int dcfm_set_probes(dcfm_handle *h, const double *V, int32_t nv, int64_t capacity) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    const Dims &d = h->d;
    if (capacity < 0) return fail(h, DCFM_ERR_INVALID, "set_probes: capacity %lld < 0", (long long)capacity);
    if (capacity > 0) {
        if (!V) return fail(h, DCFM_ERR_INVALID, "null argument");
        if (nv < 1 || nv > PROBE_NV_MAX)
            return fail(h, DCFM_ERR_INVALID, "set_probes: nv = %d outside 1..%d", (int)nv, PROBE_NV_MAX);
        for (size_t e = 0; e < (size_t)d.p * nv; ++e)
            if (!std::isfinite(V[e]))
                return fail(h, DCFM_ERR_INVALID, "set_probes: V(%zu, %zu) is not finite", e % d.p + 1, e / d.p + 1);
    }
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (h->probe_mem) (void)hipFree(h->probe_mem);
    h->probe_mem = nullptr;
    h->probes = Probes{};
    h->probe_cap = h->probe_n = 0;
    if (capacity == 0) return DCFM_OK;
    Probes pr{};
    pr.nv = nv;
    pr.slices = probe_slices(d.G);
    const size_t rows = (size_t)d.G * d.P, ts = (size_t)d.K * nv + (size_t)nv * nv;
    pr.slot = d.coll ? ts : (size_t)nv * nv;
    const size_t ntk = probe_ticket_doubles(d.G), nV = rows * nv, npart = (size_t)d.G * pr.slices * ts,
                 nterm = ((size_t)d.G + probe_groups(d.G)) * ts;
    void *q = nullptr;
    if (hipMalloc(&q, (ntk + nV + npart + nterm + (size_t)capacity * pr.slot) * sizeof(double)) != hipSuccess)
        return fail(h, DCFM_ERR_ALLOC, "set_probes: %lld draws of %d probes", (long long)capacity, (int)nv);
    h->probe_mem = static_cast<double *>(q);
    pr.ticket = reinterpret_cast<unsigned *>(h->probe_mem);
    double *dV = h->probe_mem + ntk;
    pr.V = dV;
    pr.part = dV + nV;
    pr.term = pr.part + npart;
    pr.gterm = pr.term + (size_t)d.G * ts;
    pr.draws = pr.term + nterm;
    // tickets start at 0; the upper triangles of the terms' D are never written nor read
    HIPC(h, hipMemset(h->probe_mem, 0, ntk * sizeof(double)));
    // this rank's rows of V, row-major (a loading row's nv probe entries adjacent)
    std::vector<double> loc(nV);
    const size_t row0 = (size_t)d.shard0 * d.P;
    for (size_t j = 0; j < rows; ++j)
        for (int c = 0; c < nv; ++c) loc[j * nv + c] = V[(size_t)c * d.p + row0 + j];
    HIPC(h, hipMemcpy(dV, loc.data(), nV * sizeof(double), hipMemcpyHostToDevice));
    h->probes = pr;
    h->probe_cap = capacity;
    return DCFM_OK;
}

int dcfm_get_probe_draws(dcfm_handle *h, double *out, int64_t *count) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    const Dims &d = h->d;
    const Probes &pr = h->probes;
    int code = count ? DCFM_OK : fail(h, DCFM_ERR_INVALID, "null argument");
    if (code == DCFM_OK) {
        hipError_t e = hipSetDevice(h->cfg.device);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) code = fail(h, DCFM_ERR_HIP, "get_probe_draws: %s", hipGetErrorString(e));
    }
    const size_t S = (size_t)h->probe_n, nv = (size_t)pr.nv, nq = nv * nv, mine = S * pr.slot;
    if (!d.coll || S == 0) {   // one rank: the kernel formed rho W' W + D.  No draw (on every rank): nothing to gather
        if (code != DCFM_OK) return code;
        *count = h->probe_n;
        if (out && S) HIPC(h, hipMemcpy(out, pr.draws, mine * sizeof(double), hipMemcpyDeviceToHost));
        return DCFM_OK;
    }
    // several ranks: every rank's [W_r | D_r] of all draws in one all-gather, summed in rank order
    TRY(agree(h, code));
    *count = h->probe_n;
    const size_t nr = (size_t)d.nranks, nw = (size_t)d.K * nv;
    void *q = nullptr;
    if (hipMalloc(&q, nr * mine * sizeof(double)) != hipSuccess)
        code = fail(h, DCFM_ERR_ALLOC, "get_probe_draws: gather of %zu doubles", nr * mine);
    if (int rc = agree(h, code)) {
        if (q) (void)hipFree(q);
        return rc;
    }
    double *all = static_cast<double *>(q);
    std::vector<double> host(out ? nr * mine : 0);
    int rc = coll_allgather(h, CH_MAIN, pr.draws, all, mine, h->stream);
    if (rc == DCFM_OK && out) {
        const hipError_t e = hipMemcpyAsync(host.data(), all, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) rc = fail(h, DCFM_ERR_HIP, "get_probe_draws: %s", hipGetErrorString(e));
    }
    const hipError_t es = hipStreamSynchronize(h->stream);
    (void)hipFree(all);
    if (rc == DCFM_OK && es != hipSuccess) rc = fail(h, DCFM_ERR_HIP, "get_probe_draws: %s", hipGetErrorString(es));
    if (rc != DCFM_OK || !out) return rc;
    std::vector<double> W(nw);
    for (size_t s = 0; s < S; ++s) {
        double *Q = out + s * nq;
        std::fill(W.begin(), W.end(), 0.0);
        std::fill(Q, Q + nq, 0.0);
        for (size_t r = 0; r < nr; ++r) {
            const double *t = host.data() + (r * S + s) * pr.slot;
            for (size_t e = 0; e < nw; ++e) W[e] += t[e];
            for (size_t e = 0; e < nq; ++e) Q[e] += t[nw + e];
        }
        for (size_t a = 0; a < nv; ++a)                  // one triangle, mirrored
            for (size_t b = 0; b <= a; ++b) {
                double acc = 0.0;
                for (size_t k = 0; k < (size_t)d.K; ++k) acc = std::fma(W[k * nv + a], W[k * nv + b], acc);
                Q[a * nv + b] = Q[b * nv + a] = std::fma(d.rho, acc, Q[a * nv + b]);
            }
    }
    return DCFM_OK;
}

}  // extern "C"
