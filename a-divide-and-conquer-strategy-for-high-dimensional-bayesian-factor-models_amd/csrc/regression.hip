// Posterior mean and second moment of the regression coefficients of q <= 32 response variables on all the
// others (DCFM_FLAG_REGRESSION, dcfm_set_regression / dcfm_get_regression): Bayesian factor regression.
//
// Per saved sample s, with Theta(s) = Sigma(s)^{-1}, R = (r_1 .. r_q) the responses and O their complement,
//   T(s) = Theta(s)[:, R]                    (p x q),
//   Q(s) = (T(s)[R, :] + T(s)[R, :]') / 2,   C(s) = Q(s)^{-1} = Cov[y_R | y_O, Sigma(s)]   (q x q, symmetric),
//   B(s) = -T(s) C(s), its q rows a in R set to exactly 0:  E[y_R | y_O, Sigma(s)] = B(s)' y,
//   R2_j(s) = 1 - C(s)_jj / Sigma(s)_{r_j r_j},  Sigma(s)_aa = |lambda_a(s)|^2 + omega_a(s),
// and the sums of B, B.^2, C, C.^2, R2 and R2.^2 over the saved samples are kept on the device.  B(s) is a ratio
// of entries of Theta(s), so neither moment follows from the precision mean.
//
// The columns of Theta(s) come from the four thin panels of precision_mean.hip (LeftG, LeftA, RightG, RightA; slot
// s at columns s K of each quarter of the factor buffer, written once per flush by the shared panel stage):
//   Theta(s)_ab = [a == b] / omega_a - LeftG_a . RightG_b - [a, b in one shard] LeftA_a . RightA_b,
// so for a row a outside R
//   B(s)_aj = LeftG_a . W_G[:, j] + LeftA_a . W_A[shard(a)][:, j],
//   W_G = RightG_R' C(s)  (K x q),   W_A[t] = sum_{b in R, r_b in shard t} RightA_{r_b} (x) C(s)[b, :]  (K x q).
// Two launches per flush behind the panel stage and BEFORE partial_corr.hip scales the panels in place; both only
// read the factor buffer, Lb and wslot (no hand-off between blocks, no floating-point atomics, no data-dependent
// trip count: a NaN state runs through):
//   k_reg_small  (slot): Q(s) from the response rows of the panels (k ascending), the lower triangle formed and
//                mirrored, C(s) in LDS by gj_invert and mirrored again, R2(s), W_G and the W_A of every shard that
//                holds a response into the slot's scratch, zero-padded to the MFMA k-step and to 16 columns;
//   k_reg_rows   (16 rows, 4 waves): the slots in rounds of four, one per wave: B(s)_rows on v_mfma_f64_16x16x4
//                -- the G half, then the A half once per shard of the 16 rows that holds a response, with the A
//                operand of the other rows zeroed (a 16-row tile can span several shards) -- into LDS.  Behind a
//                barrier every thread adds the round's samples to the entries it owns, in slot order.  It loads its
//                entries of the two sums first, adds one sample at a time and stores once: the bits are those of
//                a sequential sum over the saved samples, whatever asm_batch is and however the chain is cut into
//                dcfm_run calls.  (One wave per 64-row block's quarter, looping over all slots itself, left one
//                wave per SIMD waiting on its own loads: 264 us per flush at c3 against this layout's time in
//                DESIGN.md 4l.)  Block 0 adds the slots' C, C.^2, R2, R2.^2 the same way.
#include "handle.h"
#include "gj.h"

#include <set>

namespace dcfm {

constexpr int RG_ROWS = 16;        // rows of a k_reg_rows block: one MFMA tile
constexpr int RG_NW = 4;           // its waves: the slots of a round, one each
constexpr int RG_QMAX = 32;        // responses of a call
constexpr int RG_U = 8;            // k-steps of k_reg_rows whose operands are in flight together

__global__ __launch_bounds__(256) void k_reg_small(const double *__restrict__ Fb, int KH, const double *__restrict__ Lb,
                                                   int LDB, const double *__restrict__ wslot, int B, int P, int K,
                                                   Regress rg) {
    __shared__ __align__(16) double sQ[RG_QMAX * RG_QMAX];
    __shared__ __align__(16) double sCc[RG_QMAX * GJ_B];
    __shared__ int sr[RG_QMAX];
    const int s = blockIdx.x, t = threadIdx.x, q = rg.q, qp = rg.qp;
    const size_t LDF = 4 * (size_t)KH, kh = (size_t)KH, c0 = (size_t)s * K;
    if (t < q) sr[t] = rg.resp[t];
    __syncthreads();
    // Q(s): entry (i, j), j <= i, from Theta_ab and Theta_ba, mirrored
    for (int e = t; e < q * q; e += 256) {
        const int i = e / q, j = e - i * q;
        if (j > i) continue;
        const int a = sr[i], b = sr[j];
        const double *Fa = Fb + (size_t)a * LDF + c0, *Fc = Fb + (size_t)b * LDF + c0;
        double gab = 0.0, gba = 0.0, aab = 0.0, aba = 0.0;
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            gab = fma(Fa[k], Fc[2 * kh + k], gab);
            gba = fma(Fc[k], Fa[2 * kh + k], gba);
        }
        if (a / P == b / P)
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
                aab = fma(Fa[kh + k], Fc[3 * kh + k], aab);
                aba = fma(Fc[kh + k], Fa[3 * kh + k], aba);
            }
        const double dg = i == j ? 1.0 / wslot[(size_t)a * B + s] : 0.0;
        const double v = 0.5 * ((dg - gab - aab) + (dg - gba - aba));
        sQ[i * q + j] = v;
        sQ[j * q + i] = v;
    }
    (void)gj_invert(sQ, q, sCc);
    for (int e = t; e < q * q; e += 256) {                // C(s): the lower triangle, mirrored
        const int i = e / q, j = e - i * q;
        if (j > i) sQ[e] = sQ[j * q + i];
    }
    __syncthreads();
    double *sc = rg.scr + (size_t)s * rg.sstride;
    for (int e = t; e < q * q; e += 256) sc[e] = sQ[e];
    if (t < q) {                                          // R2_j = 1 - C_jj / (|lambda|^2 + omega)
        const int a = sr[t];
        const double *la = Lb + (size_t)a * LDB + c0;
        double nrm = 0.0;
        for (int k = 0; k < K; ++k) nrm = fma(la[k], la[k], nrm);
        sc[q * q + t] = 1.0 - sQ[t * q + t] / (nrm + wslot[(size_t)a * B + s]);
    }
    double *W = sc + rg.wofs;
    const size_t wsz = (size_t)rg.K4 * qp;
    for (int e = t; e < K * q; e += 256) {                // W_G = RightG_R' C, b ascending
        const int k = e / q, j = e - k * q;
        double acc = 0.0;
#pragma unroll 8
        for (int b = 0; b < q; ++b) acc = fma(Fb[(size_t)sr[b] * LDF + 2 * kh + c0 + k], sQ[b * q + j], acc);
        W[(size_t)k * qp + j] = acc;
    }
    for (int e = t; e < rg.nsh * K * q; e += 256) {       // W_A[t]: the responses of shard t, in R's order
        const int tt = e / (K * q), r = e - tt * K * q, k = r / q, j = r - k * q;
        double acc = 0.0;
        for (int u = rg.goff[tt]; u < rg.goff[tt + 1]; ++u) {
            const int b = rg.grp[u];
            acc = fma(Fb[(size_t)sr[b] * LDF + 3 * kh + c0 + k], sQ[b * q + j], acc);
        }
        W[(1 + (size_t)tt) * wsz + (size_t)k * qp + j] = acc;
    }
}

__global__ __launch_bounds__(256) void k_reg_rows(const double *__restrict__ Fb, int KH, int p, int P, int K,
                                                  int nslots, Regress rg) {
    __shared__ double sT[RG_NW][16][RG_QMAX + 1];         // a round's tiles of B(s), one per wave
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, kq = lane >> 4;
    const int q = rg.q, qp = rg.qp, nct = qp / 16, K4 = rg.K4;
    const int a0 = blockIdx.x * RG_ROWS;                  // < p: the grid is ceil(p / RG_ROWS)
    const size_t LDF = 4 * (size_t)KH, wsz = (size_t)K4 * qp;
    const int arow = min(a0 + li, p - 1), ash = arow / P;
    const bool av = a0 + li < p;
    const double *Fa = Fb + (size_t)arow * LDF;
    bool isr[4];                                          // the lane's output rows kq + 4 g: responses give exactly 0
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        isr[g] = false;
        for (int j = 0; j < q; ++j) isr[g] = isr[g] || rg.resp[j] == a0 + kq + 4 * g;
    }
    // the entries of the 16 x qp tile this thread accumulates: e = t and t + 256, row e / qp, column e % qp
    int orow[2], ocol[2];
    bool own[2];
    double sb[2], sb2[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = t + 256 * i;
        orow[i] = min(e / qp, 15);
        ocol[i] = e % qp;
        own[i] = e < 16 * qp && a0 + orow[i] < p && ocol[i] < q;
        sb[i] = own[i] ? rg.sB[(size_t)(a0 + orow[i]) * q + ocol[i]] : 0.0;
        sb2[i] = own[i] ? rg.sB2[(size_t)(a0 + orow[i]) * q + ocol[i]] : 0.0;
    }
    const int sh0 = a0 / P, sh1 = min(a0 + 15, p - 1) / P;
    for (int s0 = 0; s0 < nslots; s0 += RG_NW) {          // a round: slot s0 + wave on each wave
        const int s = s0 + wave;
        if (s < nslots) {                                 // wave-uniform: the MFMAs run with every lane
            const double *W = rg.scr + (size_t)s * rg.sstride + rg.wofs;
            const size_t c0 = (size_t)s * K;
            d4 acc[2] = {d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}};
            // acc += rows (from Frow, zero where !rowok) times Wm, k ascending; the operands of RG_U k-steps are
            // fetched before the first MFMA of the group waits for one (a load per step costs its latency per step)
            auto half = [&](const double *Frow, bool rowok, const double *Wm) {
                for (int k0 = 0; k0 < K4; k0 += 4 * RG_U) {
                    double a[RG_U], bw[RG_U][2];
#pragma unroll
                    for (int u = 0; u < RG_U; ++u) {
                        const int kk = k0 + 4 * u + kq;
                        a[u] = (rowok && kk < K) ? Frow[kk] : 0.0;
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct)
                            bw[u][ct] = (kk < K4 && ct < nct) ? Wm[(size_t)kk * qp + 16 * ct + li] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < RG_U; ++u)
                        if (k0 + 4 * u < K4)              // wave-uniform
#pragma unroll
                            for (int ct = 0; ct < 2; ++ct)
                                if (ct < nct) acc[ct] = mfma16x16x4(a[u], bw[u][ct], acc[ct]);
                }
            };
            half(Fa + c0, av, W);                         // the G half
            for (int sh = sh0; sh <= sh1; ++sh) {         // the A half, once per shard of the tile with a response
                const int tt = rg.tof[sh];
                if (tt < 0) continue;
                half(Fa + (size_t)KH + c0, av && ash == sh, W + (1 + (size_t)tt) * wsz);
            }
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (ct < nct) sT[wave][kq + 4 * g][16 * ct + li] = isr[g] ? 0.0 : acc[ct][g];
        }
        __syncthreads();
        const int nw = min(RG_NW, nslots - s0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
            for (int w = 0; w < nw; ++w) {                // the round's samples in slot order
                const double v = sT[w][orow[i]][ocol[i]];
                sb[i] += v;
                sb2[i] = fma(v, v, sb2[i]);
            }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
        if (own[i]) {
            rg.sB[(size_t)(a0 + orow[i]) * q + ocol[i]] = sb[i];
            rg.sB2[(size_t)(a0 + orow[i]) * q + ocol[i]] = sb2[i];
        }
    if (blockIdx.x == 0)                                  // [C | R2] of the slots, in slot order
        for (int e = t; e < q * q + q; e += 256) {
            double s1 = rg.sC[e], s2 = rg.sC2[e];
            for (int s = 0; s < nslots; ++s) {
                const double v = rg.scr[(size_t)s * rg.sstride + e];
                s1 += v;
                s2 = fma(v, v, s2);
            }
            rg.sC[e] = s1;
            rg.sC2[e] = s2;
        }
}

void launch_regression(const Dims &d, const Bufs &b, const PrecMean &pm, const Regress &rg, const double *Lb,
                       const double *wslot, int nslots, int B, hipStream_t s) {
    if (nslots == 0 || rg.q == 0) return;
    hipLaunchKernelGGL(k_reg_small, dim3(nslots), dim3(256), 0, s, pm.pfac, pm.KH, Lb, b.LDB, wslot, B, d.P, d.K, rg);
    hipLaunchKernelGGL(k_reg_rows, dim3(cdiv(d.p, RG_ROWS)), dim3(256), 0, s, pm.pfac, pm.KH, d.p, d.P, d.K, nslots,
                       rg);
}

}  // namespace dcfm

extern "C" {

int dcfm_set_regression(dcfm_handle *h, const int64_t *resp, int32_t q) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    if (!(h->cfg.flags & DCFM_FLAG_REGRESSION))
        return fail(h, DCFM_ERR_INVALID, "the regression coefficients need DCFM_FLAG_REGRESSION at dcfm_create");
    const Dims &d = h->d;
    if (q < 0 || q > RG_QMAX || q >= d.p)
        return fail(h, DCFM_ERR_INVALID, "set_regression: q = %d outside 0..%d, or not below p = %d", (int)q,
                    std::min(RG_QMAX, d.p - 1), d.p);
    if (q > 0 && !resp) return fail(h, DCFM_ERR_INVALID, "null argument");
    for (int j = 0; j < q; ++j) {
        if (resp[j] < 0 || resp[j] >= d.p)
            return fail(h, DCFM_ERR_INVALID, "set_regression: response %lld outside [0, %d)", (long long)resp[j], d.p);
        for (int i = 0; i < j; ++i)
            if (resp[i] == resp[j])
                return fail(h, DCFM_ERR_INVALID, "set_regression: response %lld listed twice", (long long)resp[j]);
    }
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    HIPC(h, hipStreamSynchronize(h->sasm));
    Regress rg{};
    void *mem = nullptr;
    if (q > 0) {
        // the shards that hold a response, ascending, and the responses of each in R's order
        std::set<int> shs;
        for (int j = 0; j < q; ++j) shs.insert((int)(resp[j] / d.P));
        const std::vector<int> shards(shs.begin(), shs.end());
        const int nsh = (int)shards.size();
        std::vector<int> ints;                            // [resp (q) | grp (q) | goff (nsh + 1) | tof (g)]
        for (int j = 0; j < q; ++j) ints.push_back((int)resp[j]);
        std::vector<int> goff(1, 0);
        for (int sh : shards) {
            for (int j = 0; j < q; ++j)
                if ((int)(resp[j] / d.P) == sh) ints.push_back(j);
            goff.push_back((int)ints.size() - q);
        }
        ints.insert(ints.end(), goff.begin(), goff.end());
        for (int m = 0; m < d.g; ++m) {
            const auto it = std::find(shards.begin(), shards.end(), m);
            ints.push_back(it == shards.end() ? -1 : (int)(it - shards.begin()));
        }
        rg.q = q;
        rg.qp = (q + 15) / 16 * 16;
        rg.nsh = nsh;
        rg.K4 = (d.K + 3) & ~3;
        rg.wofs = ((size_t)q * q + q + 1) & ~(size_t)1;
        rg.sstride = rg.wofs + (1 + (size_t)nsh) * rg.K4 * rg.qp;
        const size_t nscr = (size_t)h->B * rg.sstride, nb = (size_t)d.p * q, nc = (size_t)q * q + q;
        const size_t nd = nscr + 2 * nb + 2 * nc;
        if (hipMalloc(&mem, nd * sizeof(double) + ints.size() * sizeof(int)) != hipSuccess)
            return fail(h, DCFM_ERR_ALLOC, "set_regression: %d responses", (int)q);
        double *dm = static_cast<double *>(mem);
        rg.scr = dm;
        rg.sB = dm + nscr;
        rg.sB2 = rg.sB + nb;
        rg.sC = rg.sB2 + nb;
        rg.sC2 = rg.sC + nc;
        int *di = reinterpret_cast<int *>(dm + nd);
        rg.resp = di;
        rg.grp = di + q;
        rg.goff = di + 2 * q;
        rg.tof = di + 2 * q + nsh + 1;
        // the scratch's padding and the accumulators start at 0
        hipError_t e = hipMemset(mem, 0, nd * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(di, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(mem);
            return fail(h, DCFM_ERR_HIP, "set_regression: %s", hipGetErrorString(e));
        }
    }
    if (h->reg_mem) (void)hipFree(h->reg_mem);
    h->reg_mem = mem;
    h->rg = rg;
    h->reg_n = 0;
    return DCFM_OK;
}

int dcfm_get_regression(dcfm_handle *h, double *coef, double *coef_m2, double *rcov, double *rcov_m2, double *r2,
                        double *r2_m2, int64_t *count) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    if (!count) return fail(h, DCFM_ERR_INVALID, "null argument");
    *count = h->rg.q ? h->reg_n : 0;
    if (*count == 0) return DCFM_OK;
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    HIPC(h, hipStreamSynchronize(h->sasm));
    const Regress &rg = h->rg;
    const size_t p = (size_t)h->d.p, q = (size_t)rg.q, nc = q * q + q;
    const double cnt = (double)h->reg_n;                  // the samples accumulated (the population form)
    std::vector<double> host(std::max(p * q, nc));
    for (int which = 0; which < 2; ++which) {
        double *out = which ? coef_m2 : coef;
        if (out) {
            HIPC(h, hipMemcpy(host.data(), which ? rg.sB2 : rg.sB, p * q * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t a = 0; a < p; ++a)
                for (size_t j = 0; j < q; ++j) out[j * p + a] = host[a * q + j] / cnt;
        }
        double *oc = which ? rcov_m2 : rcov, *orr = which ? r2_m2 : r2;
        if (oc || orr) {
            HIPC(h, hipMemcpy(host.data(), which ? rg.sC2 : rg.sC, nc * sizeof(double), hipMemcpyDeviceToHost));
            if (oc)
                for (size_t e = 0; e < q * q; ++e) oc[e] = host[e] / cnt;
            if (orr)
                for (size_t j = 0; j < q; ++j) orr[j] = host[q * q + j] / cnt;
        }
    }
    return DCFM_OK;
}

}  // extern "C"
