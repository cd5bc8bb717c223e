// Data ingest and state I/O of the C ABI: the layout conversion between the reference's MATLAB
// column-major arrays and the device layout (dcfm_internal.h), injected draws.
#include "handle.h"

static int reset_numeric(dcfm_handle *h) {
    HIPC(h, hipMemset(h->nan_dev, 0, sizeof(int)));
    *h->nan_host = 0;
    return DCFM_OK;
}

extern "C" {

// Yd local: n x P x G column-major: (i, j, m) at i + n*j + n*P*m  ->  Y[m][i][j]
int dcfm_set_data(dcfm_handle *h, const double *Yd) {
    if (!h || !Yd) return fail(h, DCFM_ERR_INVALID, "null argument");
    const Dims &d = h->d;
    HIPC(h, hipSetDevice(h->cfg.device));
    impute_drop(h);   // dcfm_set_missing's mask belongs to the data it was given for
    std::vector<double> buf((size_t)d.NP * d.PP, 0.0);
    std::vector<double> yy((size_t)d.G * d.PP, 0.0);
    for (int m = 0; m < d.G; ++m) {
        std::fill(buf.begin(), buf.end(), 0.0);
        const double *src = Yd + (size_t)m * d.n * d.P;
        for (int j = 0; j < d.P; ++j) {
            double s = 0.0;
            for (int i = 0; i < d.n; ++i) {
                const double v = src[(size_t)j * d.n + i];
                buf[(size_t)i * d.PP + j] = v;
                s += v * v;
            }
            yy[(size_t)m * d.PP + j] = s;
        }
        HIPC(h, hipMemcpy(h->b.Y + (size_t)m * d.NP * d.PP, buf.data(), buf.size() * sizeof(double),
                          hipMemcpyHostToDevice));
    }
    HIPC(h, hipMemcpy(h->b.yy, yy.data(), yy.size() * sizeof(double), hipMemcpyHostToDevice));
    h->have_data = true;
    return DCFM_OK;
}

// device scratch freed on every return path of the ingest entry points
struct DevScratch {
    std::vector<void *> p;
    ~DevScratch() { for (void *q : p) (void)hipFree(q); }
    hipError_t alloc(void **q, size_t bytes) {
        hipError_t e = hipMalloc(q, std::max<size_t>(bytes, 1));
        if (e == hipSuccess) p.push_back(*q);
        return e;
    }
};

int dcfm_set_data_raw(dcfm_handle *h, const double *Y, int64_t p_in, const int64_t *cols, double *sd_out,
                      double *dev_ms) {
    if (!h || !Y || !cols) return fail(h, DCFM_ERR_INVALID, "null argument");
    const Dims &d = h->d;
    if (d.n < 2) return fail(h, DCFM_ERR_INVALID, "set_data_raw: var (dc:57) needs n >= 2");
    const int64_t ncols = (int64_t)d.P * d.G;
    for (int64_t c = 0; c < ncols; ++c)
        if (cols[c] < 0 || cols[c] >= p_in)
            return fail(h, DCFM_ERR_INVALID, "set_data_raw: cols[%lld] = %lld outside [0, %lld)", (long long)c,
                        (long long)cols[c], (long long)p_in);
    HIPC(h, hipSetDevice(h->cfg.device));
    impute_drop(h);   // as dcfm_set_data
    DevScratch sc;
    void *qY = nullptr, *qc = nullptr, *qsd = nullptr, *qbad = nullptr, *qmi = nullptr;
    const size_t ybytes = (size_t)d.n * (size_t)p_in * sizeof(double);
    if (sc.alloc(&qY, ybytes) != hipSuccess || sc.alloc(&qc, ncols * sizeof(int64_t)) != hipSuccess ||
        sc.alloc(&qsd, ncols * sizeof(double)) != hipSuccess || sc.alloc(&qbad, sizeof(int)) != hipSuccess ||
        sc.alloc(&qmi, 2 * ncols * sizeof(double)) != hipSuccess)
        return fail(h, DCFM_ERR_ALLOC, "set_data_raw: device scratch (%zu bytes of Y) failed", ybytes);
    hipStream_t s = h->stream;
    HIPC(h, hipMemcpyAsync(qY, Y, ybytes, hipMemcpyHostToDevice, s));
    HIPC(h, hipMemcpyAsync(qc, cols, ncols * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIPC(h, hipMemsetAsync(qbad, 0, sizeof(int), s));
    hipEvent_t ea = get_event(h), eb = get_event(h);
    if (!ea || !eb) return fail(h, DCFM_ERR_HIP, "set_data_raw: hipEventCreate failed");
    HIPC(h, hipEventRecord(ea, s));
    launch_stdize(d, static_cast<const double *>(qY), static_cast<const long long *>(qc), h->b.Y, h->b.yy,
                  static_cast<double *>(qsd), static_cast<int *>(qbad), static_cast<double *>(qmi), s);
    HIPC(h, hipGetLastError());
    HIPC(h, hipEventRecord(eb, s));
    int bad = 0;
    HIPC(h, hipMemcpyAsync(&bad, qbad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));
    if (dev_ms) {
        float ms = 0.f;
        HIPC(h, hipEventElapsedTime(&ms, ea, eb));
        *dev_ms = ms;
    }
    h->evpool.push_back(ea);
    h->evpool.push_back(eb);
    if (bad) {
        h->have_data = false;
        return fail(h, DCFM_ERR_INVALID, "a constant non-zero column has zero variance (dc:59 divides by zero, Q13)");
    }
    if (sd_out) HIPC(h, hipMemcpy(sd_out, qsd, ncols * sizeof(double), hipMemcpyDeviceToHost));
    h->have_data = true;
    return DCFM_OK;
}

int dcfm_init_state(dcfm_handle *h) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    HIPC(h, hipSetDevice(h->cfg.device));
    sync_all(h);
    launch_init_state(h->d, h->b, h->stream);
    HIPC(h, hipGetLastError());
    HIPC(h, hipStreamSynchronize(h->stream));
    h->cur = 0;
    h->plam_valid = true;      // Plam = psi o tau' was formed (dc:86), as set_state's caller Plam
    h->have_state = true;
    return reset_numeric(h);
}

int dcfm_get_data(dcfm_handle *h, double *Yd_local) {
    if (!h || !Yd_local) return fail(h, DCFM_ERR_INVALID, "null argument");
    if (!h->have_data) return fail(h, DCFM_ERR_INVALID, "get_data: no data set");
    const Dims &d = h->d;
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    std::vector<double> buf((size_t)d.NP * d.PP);
    for (int m = 0; m < d.G; ++m) {
        HIPC(h, hipMemcpy(buf.data(), h->b.Y + (size_t)m * d.NP * d.PP, buf.size() * sizeof(double),
                          hipMemcpyDeviceToHost));
        double *dst = Yd_local + (size_t)m * d.n * d.P;
        for (int j = 0; j < d.P; ++j)
            for (int i = 0; i < d.n; ++i) dst[(size_t)j * d.n + i] = buf[(size_t)i * d.PP + j];
    }
    return DCFM_OK;
}

int dcfm_count_nonzero_columns(int device, const double *Y, int32_t n, int64_t p, int32_t *nnz_out,
                               double *dev_ms) {
    if (!Y || !nnz_out || n < 0 || p < 0) return fail(nullptr, DCFM_ERR_INVALID, "count_nonzero_columns: bad argument");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, DCFM_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    DevScratch sc;
    void *qY = nullptr, *qn = nullptr;
    const size_t ybytes = (size_t)n * (size_t)p * sizeof(double);
    if (sc.alloc(&qY, ybytes) != hipSuccess || sc.alloc(&qn, (size_t)p * sizeof(int32_t)) != hipSuccess)
        return fail(nullptr, DCFM_ERR_ALLOC, "count_nonzero_columns: device scratch (%zu bytes) failed", ybytes);
    hipEvent_t ea = nullptr, eb = nullptr;
    float ms = 0.f;
    e = hipMemcpy(qY, Y, ybytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreate(&ea);
    if (e == hipSuccess) e = hipEventCreate(&eb);
    if (e == hipSuccess) e = hipEventRecord(ea, nullptr);
    if (e == hipSuccess) {
        launch_nnz_cols(static_cast<const double *>(qY), n, p, static_cast<int *>(qn), nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(eb, nullptr);
    if (e == hipSuccess) e = hipMemcpy(nnz_out, qn, (size_t)p * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ea, eb);
    if (ea) (void)hipEventDestroy(ea);
    if (eb) (void)hipEventDestroy(eb);
    if (e != hipSuccess) return fail(nullptr, DCFM_ERR_HIP, "count_nonzero_columns: %s", hipGetErrorString(e));
    if (dev_ms) *dev_ms = ms;
    return DCFM_OK;
}

// A state array on the host is MATLAB column-major (i, k, m) at i + inner * (k + K * m); on the device
// it is [m][i][k], rows padded to inner_pad and width to KW, the padding holding `fill`.  relayout copies
// one way or the other (to the device: host is only read).
struct StateLayout { int inner, inner_pad, shards, K, KW; double fill; };
static StateLayout pk_layout(const Dims &d) { return {d.P, d.PP, d.G, d.K, d.kp, 0.0}; }        // P x K x G
static StateLayout nk_layout(const Dims &d, int G) { return {d.n, d.NP, G, d.K, d.kp, 0.0}; }   // n x K x G
static StateLayout p_layout(const Dims &d) { return {d.P, d.PP, d.G, 1, 1, 0.0}; }              // P x G
static StateLayout k_layout(const Dims &d) { return {1, 1, d.g, d.K, d.kp, 1.0}; }              // K x 1 x g, pads 1
static void relayout(const StateLayout &L, bool to_device, double *host, std::vector<double> &dev) {
    if (to_device) dev.assign((size_t)L.shards * L.inner_pad * L.KW, L.fill);
    for (int m = 0; m < L.shards; ++m)
        for (int k = 0; k < L.K; ++k)
            for (int i = 0; i < L.inner; ++i) {
                double &hv = host[(size_t)i + (size_t)L.inner * k + (size_t)L.inner * L.K * m];
                double &dv = dev[((size_t)m * L.inner_pad + i) * L.KW + k];
                if (to_device) dv = hv; else hv = dv;
            }
}
static void to_dev(const StateLayout &L, const double *src, std::vector<double> &dst) { relayout(L, true, const_cast<double *>(src), dst); }
static void from_dev(const StateLayout &L, std::vector<double> &src, double *dst) { relayout(L, false, dst, src); }

static int up(dcfm_handle *h, double *dev, const std::vector<double> &v) {
    HIPC(h, hipMemcpy(dev, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    return DCFM_OK;
}
static int down(dcfm_handle *h, std::vector<double> &v, const double *dev, size_t n) {
    v.resize(n);
    HIPC(h, hipMemcpy(v.data(), dev, n * sizeof(double), hipMemcpyDeviceToHost));
    return DCFM_OK;
}

int dcfm_set_state(dcfm_handle *h, const dcfm_state_view *s) {
    if (!h || !s) return fail(h, DCFM_ERR_INVALID, "null argument");
    if (!s->Lambda || !s->ps || !s->omega || !s->psi || !s->Plam || !s->X || !s->Z || !s->delta || !s->tauh)
        return fail(h, DCFM_ERR_INVALID, "set_state: every member except eta is required");
    const Dims &d = h->d;
    HIPC(h, hipSetDevice(h->cfg.device));
    sync_all(h);
    std::vector<double> v;
    int rc;
    to_dev(pk_layout(d), s->Lambda, v); if ((rc = up(h, h->b.Lam, v))) return rc;
    to_dev(pk_layout(d), s->psi, v);    if ((rc = up(h, h->b.psi, v))) return rc;
    to_dev(pk_layout(d), s->Plam, v);   if ((rc = up(h, h->b.Plam, v))) return rc;
    to_dev(p_layout(d), s->ps, v);      if ((rc = up(h, h->b.ps, v))) return rc;
    to_dev(p_layout(d), s->omega, v);   if ((rc = up(h, h->b.omega, v))) return rc;
    to_dev(nk_layout(d, 1), s->X, v);   if ((rc = up(h, h->b.X, v))) return rc;
    to_dev(nk_layout(d, d.G), s->Z, v); if ((rc = up(h, h->b.Z, v))) return rc;
    h->cur = 0;
    to_dev(k_layout(d), s->delta, v);   if ((rc = up(h, h->b.delta, v))) return rc;
    to_dev(k_layout(d), s->tauh, v);    if ((rc = up(h, h->b.tau, v))) return rc;
    h->plam_valid = true;
    h->have_state = true;
    return reset_numeric(h);
}

static int get_state(dcfm_handle *h, dcfm_state_view *o, bool checked) {
    if (!h || !o) return fail(h, DCFM_ERR_INVALID, "null argument");
    const Dims &d = h->d;
    HIPC(h, hipSetDevice(h->cfg.device));
    sync_all(h);
    if (checked)
        if (int rc = numeric_status(h)) return rc;
    std::vector<double> v;
    int rc;
    const size_t KP = d.kp;
    const size_t npk = (size_t)d.G * d.PP * KP, nnk = (size_t)d.G * d.NP * KP;
    if (o->Lambda) { if ((rc = down(h, v, h->b.Lam, npk))) return rc; from_dev(pk_layout(d), v, o->Lambda); }
    if (o->psi) { if ((rc = down(h, v, h->b.psi, npk))) return rc; from_dev(pk_layout(d), v, o->psi); }
    if (o->Plam) {
        if (h->plam_valid) {
            if ((rc = down(h, v, h->b.Plam, npk))) return rc;
        } else {   // Plam = psi o tau' (dc:176) of the last iteration, formed as k_lambda forms it
            std::vector<double> tau;
            if ((rc = down(h, v, h->b.psi, npk))) return rc;
            if ((rc = down(h, tau, h->b.tau + h->cur * (size_t)d.g * KP, (size_t)d.g * KP))) return rc;
            for (int m = 0; m < d.G; ++m)
                for (int j = 0; j < d.P; ++j)
                    for (int k = 0; k < d.K; ++k) {
                        double &x = v[((size_t)m * d.PP + j) * KP + k];
                        x = x * tau[(size_t)(d.shard0 + m) * KP + k];
                    }
        }
        from_dev(pk_layout(d), v, o->Plam);
    }
    if (o->ps) { if ((rc = down(h, v, h->b.ps, (size_t)d.G * d.PP))) return rc; from_dev(p_layout(d), v, o->ps); }
    if (o->omega) { if ((rc = down(h, v, h->b.omega, (size_t)d.G * d.PP))) return rc; from_dev(p_layout(d), v, o->omega); }
    if (o->X) { if ((rc = down(h, v, h->b.X, (size_t)d.NP * KP))) return rc; from_dev(nk_layout(d, 1), v, o->X); }
    if (o->Z) { if ((rc = down(h, v, h->b.Z, nnk))) return rc; from_dev(nk_layout(d, d.G), v, o->Z); }
    if (o->eta) {
        launch_eta(d, h->b, h->b.W, h->stream);   // W is scratch between iterations
        HIPC(h, hipGetLastError());
        HIPC(h, hipStreamSynchronize(h->stream));
        if ((rc = down(h, v, h->b.W, nnk))) return rc;
        from_dev(nk_layout(d, d.G), v, o->eta);
    }
    const size_t nkg = (size_t)d.g * KP;
    if (o->delta) { if ((rc = down(h, v, h->b.delta + h->cur * nkg, nkg))) return rc; from_dev(k_layout(d), v, o->delta); }
    if (o->tauh) { if ((rc = down(h, v, h->b.tau + h->cur * nkg, nkg))) return rc; from_dev(k_layout(d), v, o->tauh); }
    return DCFM_OK;
}

int dcfm_get_state(dcfm_handle *h, dcfm_state_view *o) { return get_state(h, o, true); }

// forensic read after DCFM_ERR_NUMERIC: the state as the device holds it, non-finite values included
int dcfm_get_state_raw(dcfm_handle *h, dcfm_state_view *o) { return get_state(h, o, false); }

int dcfm_set_draws(dcfm_handle *h, const dcfm_draws_view *dv, int64_t first_iter, int64_t n_iter) {
    if (!h || !dv || n_iter < 1) return fail(h, DCFM_ERR_INVALID, "bad argument");
    if (!dv->NZ || !dv->NX || !dv->NL || !dv->Gpsi || !dv->Gdelta || !dv->Gps)
        return fail(h, DCFM_ERR_INVALID, "set_draws: all six arrays required");
    const Dims &d = h->d;
    HIPC(h, hipSetDevice(h->cfg.device));
    sync_all(h);
    const size_t T = n_iter;
    const size_t nNZ = (size_t)d.K * d.n * d.g * T, nNX = (size_t)d.K * d.n * T,
                 nNL = (size_t)d.K * d.P * d.g * T, nPsi = (size_t)d.P * d.K * d.g * T,
                 nDel = (size_t)d.K * d.g * T, nPs = (size_t)d.P * d.g * T;
    const size_t tot = nNZ + nNX + nNL + nPsi + nDel + nPs;
    if (h->draws_mem) { (void)hipFree(h->draws_mem); h->draws_mem = nullptr; }
    void *q = nullptr;
    HIPC(h, hipMalloc(&q, tot * sizeof(double)));
    h->draws_mem = static_cast<double *>(q);
    double *p = h->draws_mem;
    const double *srcs[6] = {dv->NZ, dv->NX, dv->NL, dv->Gpsi, dv->Gdelta, dv->Gps};
    const size_t cnt[6] = {nNZ, nNX, nNL, nPsi, nDel, nPs};
    const double **dsts[6] = {&h->dr.NZ, &h->dr.NX, &h->dr.NL, &h->dr.Gpsi, &h->dr.Gdelta, &h->dr.Gps};
    // Gpsi: MATLAB P x K x g x T -> device [T][g][P][K] (the loading-row kernels read a row's K gammas)
    std::vector<double> gpsi(nPsi);
    for (size_t t = 0; t < T; ++t)
        for (int m = 0; m < d.g; ++m)
            for (int k = 0; k < d.K; ++k)
                for (int j = 0; j < d.P; ++j)
                    gpsi[((t * d.g + m) * d.P + j) * d.K + k] = dv->Gpsi[j + (size_t)d.P * (k + (size_t)d.K * (m + (size_t)d.g * t))];
    srcs[3] = gpsi.data();
    for (int k = 0; k < 6; ++k) {
        HIPC(h, hipMemcpy(p, srcs[k], cnt[k] * sizeof(double), hipMemcpyHostToDevice));
        *dsts[k] = p;
        p += cnt[k];
    }
    h->dr.first_iter = first_iter;
    h->dr.n_iter = n_iter;
    return DCFM_OK;
}

}  // extern "C"
