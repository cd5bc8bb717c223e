// Sigmaout as a linear operator at the C ABI: dcfm_sigma_apply (Y = Sigmaout V, the kernel of
// sigma_apply.hip) and dcfm_sigma_eigs (the largest eigenpairs by a block Krylov iteration on it).
// Sigmaout never leaves HBM; the tall-skinny algebra of the iteration runs on the host, as
// dcfm_sigma_error keeps its Lanczos basis there.
#include "sigma_op.h"
#include "symeig.h"

#include <new>

namespace {

// out (p x nv column-major, host) = Sigmaout V, in blocks of <= 32 columns; collective over ranks
// (every rank's tiles, summed on CH_ASM: every rank gets the full product).  ms (nullable)
// accumulates the kernels' device time.
int apply_host(dcfm_handle *h, ApplyScratch &sc, const double *V, int nv, double *out, double *ms) {
    const Dims &d = h->d;
    const size_t P = (size_t)d.p;
    for (int c0 = 0; c0 < nv; c0 += APPLY_NB) {
        const int w = std::min(APPLY_NB, nv - c0);
        HIPC(h, hipMemcpyAsync(sc.dV, V + P * c0, P * w * sizeof(double), hipMemcpyHostToDevice, h->stream));
        const bool timed = ms && sc.ea && sc.eb;
        if (timed) HIPC(h, hipEventRecord(sc.ea, h->stream));
        launch_sigma_apply(h->b.Sigma, d.p, h->b.T0, h->b.T1, sc.dV, w, sc.part, sc.dY, h->stream);
        HIPC(h, hipGetLastError());
        if (timed) HIPC(h, hipEventRecord(sc.eb, h->stream));
        if (d.coll) TRY(coll_allreduce_sum(h, CH_ASM, sc.dY, P * w, h->stream));
        HIPC(h, hipMemcpyAsync(out + P * c0, sc.dY, P * w * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        if (timed) {
            float t = 0.f;
            HIPC(h, hipEventElapsedTime(&t, sc.ea, sc.eb));
            *ms += t;
        }
    }
    return DCFM_OK;
}

double dot(const double *a, const double *b, size_t n) {
    double acc = 0.0;
    for (size_t i = 0; i < n; ++i) acc += a[i] * b[i];
    return acc;
}

// Appends to the orthonormal basis Q (p x m column-major) the candidates C (p x nc) made orthogonal,
// twice, to the whole basis and to each other (column by column, so "within itself" is the same
// sweep); a column whose norm falls below 1e-13 of its norm before is dropped (deflation): it lies
// in the span already, and what is left of it is rounding noise.  At most `room` columns are kept.
int orth_append(std::vector<double> &Q, size_t P, const double *C, int nc, int room) {
    int kept = 0;
    std::vector<double> v(P);
    for (int c = 0; c < nc && kept < room; ++c) {
        std::copy(C + P * c, C + P * (c + 1), v.begin());
        const double n0 = std::sqrt(dot(v.data(), v.data(), P));
        if (!(n0 > 0.0) || !std::isfinite(n0)) continue;
        const size_t m = Q.size() / P;
        for (int rep = 0; rep < 2; ++rep)
            for (size_t j = 0; j < m; ++j) {
                const double *qj = Q.data() + P * j;
                const double cf = dot(v.data(), qj, P);
                for (size_t i = 0; i < P; ++i) v[i] -= cf * qj[i];
            }
        const double n1 = std::sqrt(dot(v.data(), v.data(), P));
        if (!(n1 > 1e-13 * n0)) continue;
        for (size_t i = 0; i < P; ++i) v[i] /= n1;
        Q.insert(Q.end(), v.begin(), v.end());
        ++kept;
    }
    return kept;
}

}  // namespace

extern "C" {

int dcfm_sigma_apply(dcfm_handle *h, const double *V, int32_t nv, double *out, double *dev_ms) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    int code = DCFM_OK;
    if (!V || !out) code = fail(h, DCFM_ERR_INVALID, "null argument");
    else if (nv < 1) code = fail(h, DCFM_ERR_INVALID, "sigma_apply: nv = %d < 1", nv);
    code = sigma_op_enter(h, code, "sigma_apply");
    ApplyScratch sc;
    if (code == DCFM_OK) code = sc.alloc(h, nv, "sigma_apply");   // before agree(): fails on every rank
    if (int rc = agree(h, code)) {
        sc.release(h);
        return rc;
    }
    double ms = 0.0;
    const int rc = apply_host(h, sc, V, nv, out, dev_ms ? &ms : nullptr);
    sc.release(h);
    if (rc == DCFM_OK && dev_ms) *dev_ms = ms;
    return rc;
}

int dcfm_sigma_eigs(dcfm_handle *h, int32_t r, double tol, int32_t max_passes, uint64_t seed, double *evals,
                    double *evecs, double *resid, int32_t *passes) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    const int p = h->d.p, b = std::min(APPLY_NB, p);
    const size_t P = (size_t)p;
    int code = DCFM_OK;
    if (!evals || !resid) code = fail(h, DCFM_ERR_INVALID, "null argument");
    else if (r < 1 || r > APPLY_NB || r > p) code = fail(h, DCFM_ERR_INVALID, "sigma_eigs: r = %d outside 1..min(32, p = %d)", r, p);
    else if (!(tol > 0.0)) code = fail(h, DCFM_ERR_INVALID, "sigma_eigs: tol = %g <= 0", tol);
    else if (max_passes < 1) code = fail(h, DCFM_ERR_INVALID, "sigma_eigs: max_passes = %d < 1", max_passes);
    else if (h->saved < 1) code = fail(h, DCFM_ERR_INVALID, "sigma_eigs: no saved sample yet");
    code = sigma_op_enter(h, code, "sigma_eigs");
    ApplyScratch sc;
    // basis Q and its image W = Sigmaout Q (p x m column-major, m <= mcap), reserved here so that an
    // allocation failure fails the call on every rank before the first collective
    std::vector<double> Q, W, blk, X, SX;
    const size_t mcap = code == DCFM_OK ? std::min<size_t>(P, (size_t)max_passes * b) : 0;
    if (code == DCFM_OK) code = sc.alloc(h, b, "sigma_eigs");
    if (code == DCFM_OK) {
        try {
            Q.reserve(P * mcap);
            W.reserve(P * mcap);
            blk.resize(P * b);
            X.resize(P * r);
            SX.resize(P * r);
        } catch (const std::exception &) {   // bad_alloc, or length_error of an absurd reserve
            code = fail(h, DCFM_ERR_ALLOC, "sigma_eigs: host basis of %zu x %zu doubles", P, 2 * mcap);
        }
    }
    if (int rc = agree(h, code)) {
        sc.release(h);
        return rc;
    }
    // seeded normal start block (Box-Muller: rotation-invariant), orthonormalised
    {
        uint64_t st = seed ^ 0x5DEECE66Dull;
        const size_t tot = P * b;
        for (size_t i = 0; i < tot; i += 2) {
            const double u1 = ((splitmix64(st) >> 11) + 1.0) * 0x1.0p-53, u2 = (splitmix64(st) >> 11) * 0x1.0p-53;
            const double rr = std::sqrt(-2.0 * std::log(u1));
            blk[i] = rr * std::cos(6.283185307179586 * u2);
            if (i + 1 < tot) blk[i + 1] = rr * std::sin(6.283185307179586 * u2);
        }
        orth_append(Q, P, blk.data(), b, (int)mcap);
    }
    int rc = DCFM_OK, npass = 0;
    size_t m = 0;                              // columns of Q with their image in W
    std::vector<std::vector<double>> Hc;       // H = Q' W: column j holds rows 0..j
    std::vector<double> A, th, Yv, u(P);
    // the r largest Ritz pairs of span(Q) (descending, sign fixed by the entry of largest magnitude)
    // and their residuals || Sigmaout x - lambda x || from a real pass on them; returns the largest
    auto ritz_pairs = [&]() {
        for (int i = 0; i < r; ++i) {
            const size_t col = m - 1 - i;
            double *x = X.data() + P * i;
            std::fill(x, x + P, 0.0);
            for (size_t j = 0; j < m; ++j) {
                const double y = Yv[j * m + col];
                const double *qj = Q.data() + P * j;
                for (size_t a = 0; a < P; ++a) x[a] += y * qj[a];
            }
            size_t big = 0;
            for (size_t a = 1; a < P; ++a)
                if (std::fabs(x[a]) > std::fabs(x[big])) big = a;
            if (x[big] < 0.0)
                for (size_t a = 0; a < P; ++a) x[a] = -x[a];
            evals[i] = th[col];
        }
        rc = apply_host(h, sc, X.data(), r, SX.data(), nullptr);
        double worst = 0.0;
        for (int i = 0; i < r && rc == DCFM_OK; ++i) {
            const double *x = X.data() + P * i, *sx = SX.data() + P * i;
            double acc = 0.0;
            for (size_t a = 0; a < P; ++a) {
                const double t = sx[a] - evals[i] * x[a];
                acc += t * t;
            }
            resid[i] = std::sqrt(acc);
            worst = std::max(worst, resid[i]);
        }
        return worst;
    };
    bool have = false;                         // evals / X / resid hold the pairs of the current basis
    while (rc == DCFM_OK && npass < max_passes && Q.size() / P > m) {
        const size_t m1 = Q.size() / P;
        const int nb = (int)(m1 - m);
        W.resize(P * m1);
        rc = apply_host(h, sc, Q.data() + P * m, nb, W.data() + P * m, nullptr);
        if (rc) break;
        ++npass;
        have = false;
        for (size_t j = m; j < m1; ++j) {
            Hc.emplace_back(j + 1);
            for (size_t i = 0; i <= j; ++i) Hc[j][i] = dot(Q.data() + P * i, W.data() + P * j, P);
        }
        m = m1;
        // Rayleigh-Ritz on span(Q)
        A.assign(m * m, 0.0);
        for (size_t j = 0; j < m; ++j)
            for (size_t i = 0; i <= j; ++i) A[i * m + j] = A[j * m + i] = Hc[j][i];
        if (!symeig(A.data(), (int)m, th, Yv)) {
            rc = fail(h, DCFM_ERR_NUMERIC, "sigma_eigs: the projected eigenproblem (%zu wide) did not converge", m);
            break;
        }
        if (m == P) break;                     // the basis spans everything: exact
        // || W y - theta Q y ||, the residual of a Ritz pair from what the host holds: only when it
        // passes is a device pass spent on the pairs themselves, and that pass decides
        bool conv = m >= (size_t)r;
        const double l1 = th[m - 1];
        for (int i = 0; i < r && conv; ++i) {
            const size_t col = m - 1 - i;
            std::fill(u.begin(), u.end(), 0.0);
            for (size_t j = 0; j < m; ++j) {
                const double y = Yv[j * m + col];
                const double *wj = W.data() + P * j, *qj = Q.data() + P * j;
                for (size_t a = 0; a < P; ++a) u[a] += y * (wj[a] - th[col] * qj[a]);
            }
            conv = std::sqrt(dot(u.data(), u.data(), P)) <= tol * l1;
        }
        if (conv) {
            const double worst = ritz_pairs();
            have = rc == DCFM_OK;
            if (rc || worst <= tol * evals[0]) break;
        }
        if (npass < max_passes)                // the next block: Sigmaout times the last one
            orth_append(Q, P, W.data() + P * (m - nb), nb, (int)(std::min(mcap, P) - m));
    }
    if (rc == DCFM_OK && m < (size_t)r)
        rc = fail(h, DCFM_ERR_NUMERIC, "sigma_eigs: the start block has rank %zu < r = %d", m, r);
    if (rc == DCFM_OK && !have) ritz_pairs();
    if (rc == DCFM_OK) {
        if (evecs) std::copy(X.begin(), X.end(), evecs);
        if (passes) *passes = npass;
    }
    sc.release(h);
    return rc;
}

}  // extern "C"
