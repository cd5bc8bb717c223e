// Sigmaout read-out of the C ABI: column stripes gathered to the root rank, and the error
// against a known truth without Sigmaout leaving the device.
#include "handle.h"

// Columns [col0, col0 + ncols) of one posterior moment of Sigma (DCFM_SIGMA_*), gathered to the
// root rank: the one body of dcfm_get_sigma_cols (the mean) and dcfm_get_sigma_moment_cols.  The
// moments differ only in what k_sigma_pack reads from the rank's block(s).
// src: the same read-out pointed at the precision mean (SRC_PREC: dcfm_get_precision_mean_cols; which =
// DCFM_SIGMA_MEAN), at the two moments of the partial correlations (SRC_PCORR: dcfm_get_partial_corr_cols) or at
// those of the marginal correlations (SRC_CORR: dcfm_get_corr_cols).
enum MomentSrc { SRC_SIGMA = 0, SRC_PREC, SRC_PCORR, SRC_CORR };
static const char *const PCORR_FLAG_MSG = "the partial correlations need DCFM_FLAG_PARTIAL_CORR at dcfm_create";
static const char *const CORR_FLAG_MSG = "the correlations and communalities need DCFM_FLAG_CORR at dcfm_create";
static int sigma_moment_cols(dcfm_handle *h, int which, int64_t col0, int64_t ncols, double *out, MomentSrc src = SRC_SIGMA) {
    const bool prec = src == SRC_PREC, pcorr = src == SRC_PCORR, corr = src == SRC_CORR;
    const bool unit = pcorr || corr;   // a unit diagonal per sample, and both moments of its own
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    Dims &d = h->d;
    const int root = 0;
    int code = DCFM_OK;
    double rs = 1.0;   // SD: effsamp / saved samples (the moments carry 1 / effsamp, quirk Q8)
    if (which != DCFM_SIGMA_MEAN && which != DCFM_SIGMA_M2 && which != DCFM_SIGMA_SD)
        code = fail(h, DCFM_ERR_INVALID, "sigma moment %d: DCFM_SIGMA_MEAN, _M2 or _SD", which);
    else if (prec && !h->pm.Prec)
        code = fail(h, DCFM_ERR_INVALID, "the precision mean needs DCFM_FLAG_PRECISION_MEAN at dcfm_create");
    else if (pcorr && !h->pc.PC) code = fail(h, DCFM_ERR_INVALID, "%s", PCORR_FLAG_MSG);
    else if (corr && !h->cr.C) code = fail(h, DCFM_ERR_INVALID, "%s", CORR_FLAG_MSG);
    else if (!unit && which != DCFM_SIGMA_MEAN && !h->b.Sigma2)
        code = fail(h, DCFM_ERR_INVALID, "the second moment and the standard deviation of Sigma need "
                                         "DCFM_FLAG_SIGMA_M2 at dcfm_create");
    else if (which == DCFM_SIGMA_SD && h->saved < 1)
        code = fail(h, DCFM_ERR_INVALID, "standard deviation of %s: no saved sample yet",
                    pcorr ? "the partial correlations" : corr ? "the correlations" : "Sigma");
    else if (!out && d.rank == root) code = fail(h, DCFM_ERR_INVALID, "null output on the root rank");
    else if (col0 < 0 || ncols < 0 || col0 + ncols > d.p)
        code = fail(h, DCFM_ERR_INVALID, "columns [%lld, %lld) outside 0..p = %d", (long long)col0,
                    (long long)(col0 + ncols), d.p);
    // every failure before the gather -- arguments, device, state, scratch allocation -- is folded
    // into `code` and agreed on: every rank enters the gather, or none (no rank left blocked in it)
    if (code == DCFM_OK) {
        const hipError_t e = hipSetDevice(h->cfg.device);
        if (e != hipSuccess) code = fail(h, DCFM_ERR_HIP, "get_sigma_cols: %s", hipGetErrorString(e));
    }
    sync_all(h);
    if (code == DCFM_OK) code = numeric_status(h);
    if (which == DCFM_SIGMA_SD && h->saved > 0)
        rs = ((double)h->cfg.mcmc / (double)h->cfg.thin) / (double)h->saved;
    const int nr = d.nranks;
    const long long p = d.p, c0 = col0, c1 = col0 + ncols;
    // every rank's packed-window count for this stripe (known to all ranks: no size exchange)
    std::vector<long long> cnt(nr), base(nr);
    long long tot = 0;
    const bool is_root = d.rank == root;
    void *q = nullptr;
    if (code == DCFM_OK && ncols > 0) {
        for (int k = 0; k < nr; ++k) {
            const long long R0 = std::min<long long>(p, (long long)h->Tb[k] * ASM_TILE);
            const long long R1 = std::min<long long>(p, (long long)h->Tb[k + 1] * ASM_TILE);
            cnt[k] = win_off(c1, c0, R0, R1);
            base[k] = tot;
            tot += cnt[k];
        }
        if (tot != p * ncols) code = fail(h, DCFM_ERR_INVALID, "sigma_cols: windows cover %lld of %lld", tot, p * ncols);
    }
    if (code == DCFM_OK && ncols > 0) {
        // root: [recv (all ranks' windows, own part packed in place) | dense stripe]; others: own windows
        const size_t ndev = is_root ? (nr > 1 ? 2 * (size_t)tot : (size_t)tot) : (size_t)std::max<long long>(cnt[d.rank], 1);
        const hipError_t e = hipMalloc(&q, ndev * sizeof(double));
        if (e != hipSuccess) {
            q = nullptr;
            code = fail(h, DCFM_ERR_ALLOC, "get_sigma_cols: %zu doubles of scratch: %s", ndev, hipGetErrorString(e));
        }
    }
    if (int rc = agree(h, code)) {
        if (q) (void)hipFree(q);
        return rc;
    }
    if (ncols == 0) return DCFM_OK;
    double *buf = static_cast<double *>(q);
    double *mine = is_root ? buf + base[d.rank] : buf;
    int rc = DCFM_OK;
    // R(s)_aa = 1 for every saved sample: the diagonal of both moments is the scaled count itself, its SD 0
    const double pdiag = which == DCFM_SIGMA_SD ? 0.0 : (double)h->saved / ((double)h->cfg.mcmc / (double)h->cfg.thin);
    const double *M1 = corr ? h->cr.C : pcorr ? h->pc.PC : prec ? h->pm.Prec : h->b.Sigma;
    const double *M2 = corr ? h->cr.C2 : pcorr ? h->pc.PC2 : h->b.Sigma2;
    launch_sigma_pack(M1, M2, which, rs, d.p, h->b.T0, h->b.T1, (int)col0, (int)ncols, mine, h->stream,
                      unit ? &pdiag : nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = fail(h, DCFM_ERR_HIP, "sigma_pack: %s", hipGetErrorString(e));
    double *dense = buf;   // one rank: its windows are the dense stripe
    if (rc == DCFM_OK && nr > 1) {
        rc = coll_gather(h, mine, buf, base, cnt, root, h->stream);
        if (rc == DCFM_OK && is_root) {
            dense = buf + tot;
            void *qt = nullptr;
            e = hipMalloc(&qt, (size_t)nr * sizeof(long long) + (size_t)(nr + 1) * sizeof(int));
            if (e == hipSuccess) {
                long long *dbase = static_cast<long long *>(qt);
                int *dTb = reinterpret_cast<int *>(dbase + nr);
                e = hipMemcpyAsync(dbase, base.data(), nr * sizeof(long long), hipMemcpyHostToDevice, h->stream);
                if (e == hipSuccess)
                    e = hipMemcpyAsync(dTb, h->Tb.data(), (nr + 1) * sizeof(int), hipMemcpyHostToDevice, h->stream);
                if (e == hipSuccess) {
                    launch_sigma_unpack(buf, d.p, (int)col0, (int)ncols, dTb, dbase, nr, dense, h->stream);
                    e = hipGetLastError();
                }
                if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
                (void)hipFree(qt);
            }
            if (e != hipSuccess) rc = fail(h, DCFM_ERR_HIP, "sigma_unpack: %s", hipGetErrorString(e));
        }
    }
    if (rc == DCFM_OK && is_root) {
        e = hipMemcpyAsync(out, dense, (size_t)tot * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) rc = fail(h, DCFM_ERR_HIP, "get_sigma_cols: %s", hipGetErrorString(e));
    }
    if (rc == DCFM_OK) {
        e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(h, DCFM_ERR_HIP, "get_sigma_cols: %s", hipGetErrorString(e));
    }
    (void)hipFree(buf);
    return rc;
}

// the whole p x p moment in column stripes of <= 2 GiB
static int sigma_moment(dcfm_handle *h, int which, double *out, MomentSrc src = SRC_SIGMA) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    if (src == SRC_PREC && !h->pm.Prec)
        return fail(h, DCFM_ERR_INVALID, "the precision mean needs DCFM_FLAG_PRECISION_MEAN at dcfm_create");
    if (src == SRC_PCORR && !h->pc.PC) return fail(h, DCFM_ERR_INVALID, "%s", PCORR_FLAG_MSG);
    if (src == SRC_CORR && !h->cr.C) return fail(h, DCFM_ERR_INVALID, "%s", CORR_FLAG_MSG);
    if (!out && h->d.rank == 0) return fail(h, DCFM_ERR_INVALID, "null output on the root rank");
    const int64_t p = h->d.p;
    const int64_t chunk = std::max<int64_t>(32, std::min<int64_t>(p, ((int64_t)1 << 28) / p));
    for (int64_t c = 0; c < p; c += chunk) {
        const int rc = sigma_moment_cols(h, which, c, std::min(chunk, p - c), out ? out + (size_t)c * p : nullptr, src);
        if (rc) return rc;
    }
    return DCFM_OK;
}

extern "C" {

int dcfm_get_sigma_cols(dcfm_handle *h, int64_t col0, int64_t ncols, double *out) {
    return sigma_moment_cols(h, DCFM_SIGMA_MEAN, col0, ncols, out);
}

int dcfm_get_sigma_moment_cols(dcfm_handle *h, int32_t which, int64_t col0, int64_t ncols, double *out) {
    return sigma_moment_cols(h, which, col0, ncols, out);
}

int dcfm_get_sigma(dcfm_handle *h, double *out) { return sigma_moment(h, DCFM_SIGMA_MEAN, out); }

int dcfm_get_sigma_moment(dcfm_handle *h, int32_t which, double *out) { return sigma_moment(h, which, out); }

int dcfm_get_precision_mean_cols(dcfm_handle *h, int64_t col0, int64_t ncols, double *out) {
    return sigma_moment_cols(h, DCFM_SIGMA_MEAN, col0, ncols, out, SRC_PREC);
}

int dcfm_get_precision_mean(dcfm_handle *h, double *out) { return sigma_moment(h, DCFM_SIGMA_MEAN, out, SRC_PREC); }

int dcfm_get_partial_corr_cols(dcfm_handle *h, int32_t which, int64_t col0, int64_t ncols, double *out) {
    return sigma_moment_cols(h, which, col0, ncols, out, SRC_PCORR);
}

int dcfm_get_partial_corr(dcfm_handle *h, int32_t which, double *out) { return sigma_moment(h, which, out, SRC_PCORR); }

int dcfm_get_corr_cols(dcfm_handle *h, int32_t which, int64_t col0, int64_t ncols, double *out) {
    return sigma_moment_cols(h, which, col0, ncols, out, SRC_CORR);
}

int dcfm_get_corr(dcfm_handle *h, int32_t which, double *out) { return sigma_moment(h, which, out, SRC_CORR); }

// Every rank holds all p communalities (k_corr_scale runs over the gathered batch): no collective, each rank
// reads its own copy.  The SD is formed on the host from the two p-vectors.
int dcfm_get_communality(dcfm_handle *h, int32_t which, double *out) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    if (which != DCFM_SIGMA_MEAN && which != DCFM_SIGMA_M2 && which != DCFM_SIGMA_SD)
        return fail(h, DCFM_ERR_INVALID, "communality moment %d: DCFM_SIGMA_MEAN, _M2 or _SD", which);
    if (!h->cr.H) return fail(h, DCFM_ERR_INVALID, "%s", CORR_FLAG_MSG);
    if (which == DCFM_SIGMA_SD && h->saved < 1)
        return fail(h, DCFM_ERR_INVALID, "standard deviation of the communalities: no saved sample yet");
    if (!out) return fail(h, DCFM_ERR_INVALID, "null output");
    HIPC(h, hipSetDevice(h->cfg.device));
    sync_all(h);
    TRY(numeric_status(h));
    const size_t p = (size_t)h->d.p;
    if (which != DCFM_SIGMA_SD) {
        HIPC(h, hipMemcpy(out, which == DCFM_SIGMA_MEAN ? h->cr.H : h->cr.H2, p * sizeof(double), hipMemcpyDeviceToHost));
        return DCFM_OK;
    }
    std::vector<double> m2(p);
    HIPC(h, hipMemcpy(out, h->cr.H, p * sizeof(double), hipMemcpyDeviceToHost));
    HIPC(h, hipMemcpy(m2.data(), h->cr.H2, p * sizeof(double), hipMemcpyDeviceToHost));
    const double rs = ((double)h->cfg.mcmc / (double)h->cfg.thin) / (double)h->saved;
    for (size_t a = 0; a < p; ++a) {   // k_sigma_pack's form: sqrt(max(0, rs H2 - (rs H)^2))
        const double m = rs * out[a];
        out[a] = std::sqrt(std::fmax(0.0, std::fma(rs, m2[a], -m * m)));
    }
    return DCFM_OK;
}

int dcfm_sigma_block(const dcfm_handle *h, int64_t out[3]) {
    if (!h || !out) return fail(nullptr, DCFM_ERR_INVALID, "null argument");
    const int64_t p = h->d.p;
    out[0] = std::min<int64_t>(p, (int64_t)h->b.T0 * ASM_TILE);
    out[1] = std::min<int64_t>(p, (int64_t)h->b.T1 * ASM_TILE);
    // beside the mean: the second moment, the precision mean, the two moments of the partial correlations and of
    // the correlations
    out[2] = (int64_t)(tri(h->b.T1) - tri(h->b.T0)) * ASM_TILE * ASM_TILE * (int64_t)sizeof(double) *
             (1 + (h->b.Sigma2 ? 1 : 0) + (h->pm.Prec ? 1 : 0) + (h->pc.PC ? 2 : 0) + (h->cr.C ? 2 : 0));
    return DCFM_OK;
}

// ---------------------------------------------------------------------------
// Error of Sigmaout against a truth U U' + diag(s) (north_star
// check 2), without Sigmaout leaving the device.  Frobenius norms come from the first
// pass of k_sigma_err; the operator norm of M = Sigmaout - Sigma0 is the largest
// |eigenvalue| of the Lanczos tridiagonal T_m (symmetric M; full reorthogonalisation,
// twice, on the host: p x m doubles), found by Sturm-sequence bisection.
// ---------------------------------------------------------------------------
static int sturm_below(const std::vector<double> &a, const std::vector<double> &b, double x) {
    int cnt = 0;
    double q = 1.0;
    for (size_t i = 0; i < a.size(); ++i) {
        q = a[i] - x - (i ? b[i - 1] * b[i - 1] / q : 0.0);
        if (q == 0.0) q = -1e-300;
        if (q < 0.0) ++cnt;
    }
    return cnt;
}
static double tridiag_extreme(const std::vector<double> &a, const std::vector<double> &b, bool largest) {
    const size_t m = a.size();
    double lo = 0.0, hi = 0.0;
    for (size_t i = 0; i < m; ++i) {   // Gershgorin interval
        const double rad = (i ? std::fabs(b[i - 1]) : 0.0) + (i + 1 < m ? std::fabs(b[i]) : 0.0);
        lo = i ? std::min(lo, a[i] - rad) : a[i] - rad;
        hi = i ? std::max(hi, a[i] + rad) : a[i] + rad;
    }
    for (int it = 0; it < 200 && hi - lo > 0.0; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi) break;
        const int c = sturm_below(a, b, mid);
        if (largest ? (c == (int)m) : (c >= 1)) hi = mid;
        else lo = mid;
    }
    return 0.5 * (lo + hi);
}

int dcfm_sigma_error(dcfm_handle *h, const double *U, int32_t r, const double *sdiag, int32_t iters,
                     uint64_t seed, double out[3]) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    int code = DCFM_OK;
    if (!sdiag || !out || (r > 0 && !U)) code = fail(h, DCFM_ERR_INVALID, "null argument");
    else if (r < 0 || r > 32) code = fail(h, DCFM_ERR_INVALID, "truth rank r = %d outside 0..32", r);
    else if (iters < 0) code = fail(h, DCFM_ERR_INVALID, "iters = %d < 0", iters);
    if (code == DCFM_OK) {
        const hipError_t e = hipSetDevice(h->cfg.device);
        if (e != hipSuccess) code = fail(h, DCFM_ERR_HIP, "sigma_error: %s", hipGetErrorString(e));
    }
    sync_all(h);
    if (code == DCFM_OK) code = numeric_status(h);
    const Dims &d = h->d;
    const int p = d.p;
    const size_t P = (size_t)p;
    const int m = std::min<int>(iters, p);
    double *dev = nullptr;
    const size_t ns = (size_t)sigma_err_splits(p);
    if (code == DCFM_OK) {   // scratch before agree(): an allocation failure fails the call on every rank
        void *q = nullptr;
        const size_t nd = P * (size_t)std::max(r, 1) + 5 * P + 3 * ns * P;
        const hipError_t e = hipMalloc(&q, nd * sizeof(double));
        if (e != hipSuccess) code = fail(h, DCFM_ERR_ALLOC, "sigma_error: %zu doubles of scratch: %s", nd, hipGetErrorString(e));
        else dev = static_cast<double *>(q);
    }
    if (int rc = agree(h, code)) {   // the all-reduces below run on every rank, or on none
        if (dev) (void)hipFree(dev);
        return rc;
    }
    // U, s, v, then the summed outputs y | fro | tru (contiguous), then the split partials
    double *dU = dev, *ds = dU + P * std::max(r, 1), *dv = ds + P, *dy = dv + P, *dfro = dy + P, *dtru = dfro + P;
    double *py = dtru + P, *pfro = py + ns * P, *ptru = pfro + ns * P;
    int rc = DCFM_OK;
    auto hip_ok = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == DCFM_OK) rc = fail(h, DCFM_ERR_HIP, "sigma_error %s: %s", what, hipGetErrorString(e));
        return rc == DCFM_OK;
    };
    if (r > 0) hip_ok(hipMemcpy(dU, U, P * r * sizeof(double), hipMemcpyHostToDevice), "upload U");
    hip_ok(hipMemcpy(ds, sdiag, P * sizeof(double), hipMemcpyHostToDevice), "upload s");
    std::vector<double> V, y(P), fro(P), tru(P), alpha, beta;
    // one pass: y = M v (v may be null: norms only); collective over ranks
    auto pass = [&](const double *vh, bool first) {
        if (rc) return false;
        if (vh && !hip_ok(hipMemcpyAsync(dv, vh, P * sizeof(double), hipMemcpyHostToDevice, h->stream), "upload v"))
            return false;
        launch_sigma_err(h->b.Sigma, p, dU, r, ds, vh ? dv : nullptr, h->b.T0, h->b.T1, first, vh ? py : nullptr,
                         pfro, ptru, dy, h->stream);
        if (!hip_ok(hipGetLastError(), "launch")) return false;
        if (d.coll) {
            if (vh && (rc = coll_allreduce_sum(h, CH_ASM, dy, P, h->stream))) return false;
            if (first && (rc = coll_allreduce_sum(h, CH_ASM, dfro, P, h->stream))) return false;
            if (first && (rc = coll_allreduce_sum(h, CH_ASM, dtru, P, h->stream))) return false;
        }
        if (vh) hip_ok(hipMemcpyAsync(y.data(), dy, P * sizeof(double), hipMemcpyDeviceToHost, h->stream), "y");
        if (first) {
            hip_ok(hipMemcpyAsync(fro.data(), dfro, P * sizeof(double), hipMemcpyDeviceToHost, h->stream), "fro");
            hip_ok(hipMemcpyAsync(tru.data(), dtru, P * sizeof(double), hipMemcpyDeviceToHost, h->stream), "tru");
        }
        return hip_ok(hipStreamSynchronize(h->stream), "sync");
    };
    auto dot = [&](const double *a, const double *b) {
        double acc = 0.0;
        for (size_t i = 0; i < P; ++i) acc += a[i] * b[i];
        return acc;
    };
    if (m == 0) {
        pass(nullptr, true);
    } else {
        V.assign(P * (size_t)(m + 1), 0.0);
        uint64_t st = seed ^ 0x5DEECE66Dull;
        for (size_t i = 0; i < P; i += 2) {   // Box-Muller normals: a rotation-invariant start
            const double u1 = ((splitmix64(st) >> 11) + 1.0) * 0x1.0p-53, u2 = (splitmix64(st) >> 11) * 0x1.0p-53;
            const double rr = std::sqrt(-2.0 * std::log(u1));
            V[i] = rr * std::cos(6.283185307179586 * u2);
            if (i + 1 < P) V[i + 1] = rr * std::sin(6.283185307179586 * u2);
        }
        const double n0 = std::sqrt(dot(V.data(), V.data()));
        for (size_t i = 0; i < P; ++i) V[i] /= n0;
        double bprev = 0.0;
        for (int j = 0; j < m; ++j) {
            double *vj = V.data() + P * j, *vn = V.data() + P * (j + 1);
            if (!pass(vj, j == 0)) break;
            const double a = dot(y.data(), vj);
            const double *vp = j ? vj - P : vj;
            const double bp = j ? bprev : 0.0;
            for (size_t i = 0; i < P; ++i) vn[i] = y[i] - a * vj[i] - bp * vp[i];
            for (int rep = 0; rep < 2; ++rep)
                for (int i2 = 0; i2 <= j; ++i2) {
                    const double *vi = V.data() + P * i2;
                    const double c = dot(vn, vi);
                    for (size_t i = 0; i < P; ++i) vn[i] -= c * vi[i];
                }
            const double bn = std::sqrt(dot(vn, vn));
            alpha.push_back(a);
            double scale = std::fabs(a);
            for (double x : alpha) scale = std::max(scale, std::fabs(x));
            if (bn <= 1e-13 * std::max(scale, 1e-300)) break;   // invariant subspace: T is exact
            beta.push_back(bn);
            for (size_t i = 0; i < P; ++i) vn[i] /= bn;
            bprev = bn;
        }
    }
    if (rc == DCFM_OK) {
        double fs = 0.0, ts = 0.0;
        for (size_t i = 0; i < P; ++i) {
            fs += fro[i];
            ts += tru[i];
        }
        out[0] = std::sqrt(fs);
        out[1] = std::sqrt(ts);
        out[2] = 0.0;
        if (!alpha.empty()) {
            beta.resize(alpha.size() - 1);
            out[2] = std::max(std::fabs(tridiag_extreme(alpha, beta, true)),
                              std::fabs(tridiag_extreme(alpha, beta, false)));
        }
    }
    (void)hipFree(dev);
    return rc;
}

}  // extern "C"
