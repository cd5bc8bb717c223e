// Missing training data (dcfm_set_missing / dcfm_get_imputed): one data-augmentation step per Gibbs iteration.
// Given eta, Lambda and ps every missing entry is conditionally independent,
//   Y_ij | . ~ N(eta_i . lambda_j, 1 / ps_j),   eta_i = sqrt(rho) X_i + sqrt(1 - rho) Z_mi,
// so behind the loading rows of iteration t (X, Z, Lambda, ps of t final) the step redraws the missing entries in
// place in Y and rewrites yy of their columns; every other kernel keeps reading Y and yy from HBM as it does
// without a mask, and iteration t + 1 is an ordinary sweep on the completed matrix.  The Rao-Blackwellised
// by-products, accumulated on the saved iterations, are the posterior mean of mu_ij = eta_i . lambda_j and, by
// the law of total variance, the predictive variance avg 1 / ps_j + var mu_ij of every missing entry.
//
// Two launches on the sweep stream:
//   k_impute     one lane per missing entry of the list sorted by (local shard, row i, column j), so that the lanes
//                of a wave share their X and Z rows (a shard's Lambda stays in L2).  Each lane runs its own K-long
//                FMA chain in k order and draws its own normal, so no bit depends on the grid.  z is the Philox
//                normal at (SITE_IMPUTE, global shard, row j, index i, iteration): what dcfm_rng_fill_rows(site 13,
//                shard, iteration, rows P, width n) gives at out[j n + i].  The value goes to Y[m][i][j] and to
//                vcsc, the compact copy in (shard, column, row) order; on an accumulated sample the lane adds mu
//                and mu^2 to its own two cells.
//                The Lambda rows go through LDS.  Read straight from L2, 16 bytes per lane and k step, a wave
//                instruction touches 64 cache lines and each line comes back up to eight times (measured 1.5 - 2 x
//                slower).  Instead the wave fetches its 64 rows in 16-column chunks, 8 lanes to an
//                entry's 128-byte chunk (one cache line, read once, 8 entries per load instruction), parks them
//                in its own LDS tile, and every lane walks its own row there: the chain's operands and their
//                order are those of the direct read.
//   k_impute_yy  one wave per column with a missing entry: the squares of its contiguous vcsc segment summed
//                lane-strided (lane l takes l, l + 64, ..) and then over the wave by the xor butterfly 32, 16, .., 1,
//                an order fixed by the segment alone; yy_j = yyobs_j + that sum -- never an increment of the old
//                yy_j, whose rounding would drift over a long chain -- and on an accumulated sample snv += 1 / ps_j.
// No floating-point atomics, every cell owned by one thread, one sample added per launch in sample order: the
// same inputs give the same bits however a run is cut into calls.  A NaN state runs through to NaN entries.
#include "handle.h"
#include "philox.h"
#include "linalg.h"

#include <climits>

namespace dcfm {

constexpr int IMP_KC = 16;            // columns per staged chunk: 128 bytes of a Lambda row
constexpr int IMP_LD = IMP_KC + 2;    // tile row stride in doubles (rows stay 16-byte aligned)

__global__ __launch_bounds__(256) void k_impute(Dims d, const double *__restrict__ X, const double *__restrict__ Z,
                                                const double *__restrict__ Lam, const double *__restrict__ ps,
                                                double *__restrict__ Y, Impute im, uint32_t iter, int acc) {
    __shared__ __align__(16) double tile[4][64][IMP_LD];
    const int lane = threadIdx.x & 63, sub = lane & 7, grp = lane >> 3;
    double(*T)[IMP_LD] = tile[threadIdx.x >> 6];
    const int e0 = blockIdx.x * 256 + threadIdx.x;
    const bool live = e0 < im.nmiss;
    const int e = live ? e0 : im.nmiss - 1;               // a padding lane redoes the last entry and stores nothing
    const int i = im.row[e], jc = im.col[e], m = jc / d.PP, j = jc - m * d.PP;
    const double2 *x = reinterpret_cast<const double2 *>(X + (size_t)i * d.kp);
    const double2 *z = reinterpret_cast<const double2 *>(Z + ((size_t)m * d.NP + i) * d.kp);
    double mu = 0.0;
    for (int k0 = 0; k0 < d.K; k0 += IMP_KC) {            // the same trip count for the whole block
#pragma unroll
        for (int t = 0; t < 8; ++t) {                     // the chunk of entries 8 t .. 8 t + 7 of this wave
            const int src = 8 * t + grp;
            const int jcs = __shfl(jc, src, 64);
            const double2 v = *reinterpret_cast<const double2 *>(Lam + (size_t)jcs * d.kp + k0 + 2 * sub);
            *reinterpret_cast<double2 *>(&T[src][2 * sub]) = v;
        }
        __syncthreads();
        const int kn = min(IMP_KC, d.K - k0);
        for (int k = 0; k < kn; k += 2) {                 // k ascending; the padding columns are never read into mu
            const double2 xv = x[(k0 + k) >> 1], zv = z[(k0 + k) >> 1];
            const double2 lv = *reinterpret_cast<const double2 *>(&T[lane][k]);
            mu = fma(eta_of(d.sr, d.s1r, xv.x, zv.x), lv.x, mu);
            if (k + 1 < kn) mu = fma(eta_of(d.sr, d.s1r, xv.y, zv.y), lv.y, mu);
        }
        __syncthreads();
    }
    double n0, n1;
    Rng(d.seed).normal2(SITE_IMPUTE, (uint32_t)(d.shard0 + m), (uint32_t)j, (uint32_t)i >> 1, iter, n0, n1);
    const double v = mu + ((i & 1) ? n1 : n0) / sqrt(ps[jc]);
    if (!live) return;
    Y[((size_t)m * d.NP + i) * d.PP + j] = v;
    im.vcsc[im.perm[e]] = v;
    if (acc) {
        im.smu[e] += mu;
        im.smu2[e] = fma(mu, mu, im.smu2[e]);
    }
}

// the start values of dcfm_set_missing into Y (vcsc holds them)
__global__ __launch_bounds__(256) void k_impute_start(Dims d, double *__restrict__ Y, Impute im) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= im.nmiss) return;
    const int i = im.row[e], jc = im.col[e], m = jc / d.PP, j = jc - m * d.PP;
    Y[((size_t)m * d.NP + i) * d.PP + j] = im.vcsc[im.perm[e]];
}

__global__ __launch_bounds__(256) void k_impute_yy(const double *__restrict__ ps, double *__restrict__ yy, Impute im,
                                                   int acc) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= im.ncol) return;                             // the whole wave
    const int lo = im.colptr[c], hi = im.colptr[c + 1];
    double s = 0.0;
    for (int q = lo + lane; q < hi; q += 64) s = fma(im.vcsc[q], im.vcsc[q], s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
        const int jc = im.cols[c];
        yy[jc] = im.yyobs[c] + s;
        if (acc) im.snv[c] += 1.0 / ps[jc];
    }
}

void launch_impute(const Dims &d, const Bufs &b, const Impute &im, int64_t iter, bool acc, hipStream_t s) {
    hipLaunchKernelGGL(k_impute, dim3(cdiv(im.nmiss, 256)), dim3(256), 0, s, d, b.X, b.Z, b.Lam, b.ps, b.Y, im,
                       (uint32_t)iter, acc ? 1 : 0);
    hipLaunchKernelGGL(k_impute_yy, dim3(cdiv(im.ncol, 4)), dim3(256), 0, s, b.ps, b.yy, im, acc ? 1 : 0);
}

}  // namespace dcfm

// yy of the mask's columns as dcfm_set_data forms it (one sum over all rows in row order) from the Y the device
// holds: turning the feature off leaves the handle as if the completed matrix had been passed to dcfm_set_data
static int restore_yy(dcfm_handle *h) {
    const Dims &d = h->d;
    const Impute &im = h->imp;
    std::vector<int> cols(im.ncol);
    std::vector<double> yy((size_t)d.G * d.PP), buf((size_t)d.NP * d.PP);
    HIPC(h, hipMemcpy(cols.data(), im.cols, cols.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPC(h, hipMemcpy(yy.data(), h->b.yy, yy.size() * sizeof(double), hipMemcpyDeviceToHost));
    int held = -1;
    for (int jc : cols) {                                 // ascending in the shard
        const int m = jc / d.PP, j = jc - m * d.PP;
        if (m != held) {
            HIPC(h, hipMemcpy(buf.data(), h->b.Y + (size_t)m * d.NP * d.PP, buf.size() * sizeof(double),
                              hipMemcpyDeviceToHost));
            held = m;
        }
        double s = 0.0;
        for (int i = 0; i < d.n; ++i) s += buf[(size_t)i * d.PP + j] * buf[(size_t)i * d.PP + j];
        yy[jc] = s;
    }
    HIPC(h, hipMemcpy(h->b.yy, yy.data(), yy.size() * sizeof(double), hipMemcpyHostToDevice));
    return DCFM_OK;
}

void impute_drop(dcfm_handle *h) {
    if (!h->imp_mem) return;
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(h->imp_mem);
    h->imp_mem = nullptr;
    h->imp = Impute{};
    h->imp_cap = h->imp_n = 0;
}

extern "C" {

int dcfm_set_missing(dcfm_handle *h, const uint8_t *mask_local, int64_t capacity) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    const Dims &d = h->d;
    if (capacity < 0) return fail(h, DCFM_ERR_INVALID, "set_missing: capacity %lld < 0", (long long)capacity);
    if (!h->have_data) return fail(h, DCFM_ERR_INVALID, "set_missing: set_data first (the mask belongs to the data)");
    const size_t n = d.n, P = d.P, G = d.G, PP = d.PP;
    int64_t nm = 0;
    if (mask_local)
        for (size_t q = 0; q < n * P * G; ++q) nm += mask_local[q] != 0;
    if (nm > INT_MAX)
        return fail(h, DCFM_ERR_UNSUPPORTED, "set_missing: %lld missing entries on this rank, at most %d",
                    (long long)nm, INT_MAX);
    // the read-out of dcfm_set_loglik would be the completed-data likelihood, not the observed-data one
    if (nm > 0 && h->ll_cap > 0)
        return fail(h, DCFM_ERR_UNSUPPORTED, "set_missing: the handle records the rows' log-likelihood (dcfm_set_loglik), "
                                             "which with a mask would be that of the completed data; turn it off first");
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (nm == 0) {                                        // off
        if (h->imp_mem) TRY(restore_yy(h));
        impute_drop(h);
        return DCFM_OK;
    }
    // the two orders of the entry list, the start values and the observed sums of squares
    std::vector<int> ci(nm), cj(nm), row(nm), col(nm), perm(nm), colptr, cols, pos(n + 1);
    std::vector<double> v(nm), yyobs, buf((size_t)d.NP * PP);
    size_t q = 0;
    for (size_t m = 0; m < G; ++m) {
        HIPC(h, hipMemcpy(buf.data(), h->b.Y + m * d.NP * PP, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
        const size_t q0 = q;
        std::fill(pos.begin(), pos.end(), 0);
        for (size_t j = 0; j < P; ++j) {
            const uint8_t *mk = mask_local + (m * P + j) * n;
            const size_t qc = q;
            double so = 0.0;
            for (size_t i = 0; i < n; ++i) {
                const double x = buf[i * PP + j];
                if (!mk[i]) { so += x * x; continue; }    // a direct sum over the observed entries, in row order
                v[q] = std::isfinite(x) ? x : 0.0;        // NaN from the caller: the standardised column mean
                ci[q] = (int)i;
                cj[q] = (int)(m * PP + j);
                pos[i + 1] += 1;
                ++q;
            }
            if (q > qc) {
                colptr.push_back((int)qc);
                cols.push_back((int)(m * PP + j));
                yyobs.push_back(so);
            }
        }
        for (size_t i = 0; i < n; ++i) pos[i + 1] += pos[i];          // stable by row: columns ascend inside a row
        for (size_t c = q0; c < q; ++c) {
            const size_t e = q0 + pos[ci[c]]++;
            row[e] = ci[c];
            col[e] = cj[c];
            perm[e] = (int)c;
        }
    }
    colptr.push_back((int)nm);
    const size_t ncol = cols.size(), nacc = capacity > 0 ? 2 * (size_t)nm + ncol : 0;
    const size_t nd = (size_t)nm + ncol + nacc, ni = 3 * (size_t)nm + 2 * ncol + 1;
    void *mem = nullptr;
    if (hipMalloc(&mem, nd * sizeof(double) + ni * sizeof(int)) != hipSuccess)
        return fail(h, DCFM_ERR_ALLOC, "set_missing: %lld missing entries, %lld samples", (long long)nm, (long long)capacity);
    Impute im{};
    im.nmiss = (int)nm;
    im.ncol = (int)ncol;
    double *dp = static_cast<double *>(mem);
    im.vcsc = dp;
    im.yyobs = dp + nm;
    if (capacity > 0) {
        im.smu = im.yyobs + ncol;
        im.smu2 = im.smu + nm;
        im.snv = im.smu2 + nm;
    }
    int *ip = reinterpret_cast<int *>(dp + nd);
    int *drow = ip, *dcol = ip + nm, *dperm = ip + 2 * nm, *dcolptr = ip + 3 * nm, *dcols = dcolptr + ncol + 1;
    im.row = drow; im.col = dcol; im.perm = dperm; im.colptr = dcolptr; im.cols = dcols;
    hipError_t e = hipMemcpy(im.vcsc, v.data(), nm * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(im.yyobs, yyobs.data(), ncol * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && nacc) e = hipMemset(im.smu, 0, nacc * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(drow, row.data(), nm * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dcol, col.data(), nm * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dperm, perm.data(), nm * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dcolptr, colptr.data(), (ncol + 1) * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dcols, cols.data(), ncol * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(mem);
        return fail(h, DCFM_ERR_HIP, "set_missing: %s", hipGetErrorString(e));
    }
    // from here on the setting changes: yy of the previous mask's columns back to dcfm_set_data's form, then the
    // start values into Y and yy of the new mask's columns by the step's own kernel
    if (h->imp_mem) {
        if (int rc = restore_yy(h)) { (void)hipFree(mem); return rc; }
        impute_drop(h);
    }
    h->imp_mem = mem;
    h->imp = im;
    h->imp_cap = capacity;
    h->imp_n = 0;
    hipLaunchKernelGGL(k_impute_start, dim3(cdiv(im.nmiss, 256)), dim3(256), 0, h->stream, d, h->b.Y, im);
    hipLaunchKernelGGL(k_impute_yy, dim3(cdiv(im.ncol, 4)), dim3(256), 0, h->stream, h->b.ps, h->b.yy, im, 0);
    HIPC(h, hipGetLastError());
    HIPC(h, hipStreamSynchronize(h->stream));
    return DCFM_OK;
}

int dcfm_get_imputed(dcfm_handle *h, double *mean, double *m2, double *nvar, int64_t *count) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    if (!count) return fail(h, DCFM_ERR_INVALID, "null argument");
    const Dims &d = h->d;
    const Impute &im = h->imp;
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    *count = h->imp_n;
    if (h->imp_n == 0 || !(mean || m2 || nvar)) return DCFM_OK;
    const double cnt = (double)h->imp_n;                  // the samples accumulated (the population form)
    const size_t n = d.n, P = d.P, G = d.G, PP = d.PP, nm = im.nmiss, ncol = im.ncol;
    if (mean || m2) {
        std::vector<double> buf((size_t)d.NP * PP), s1(nm), s2(nm);
        std::vector<int> row(nm), col(nm);
        for (size_t m = 0; m < G; ++m) {                  // the observed positions: Y and Y^2
            HIPC(h, hipMemcpy(buf.data(), h->b.Y + m * d.NP * PP, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t j = 0; j < P; ++j)
                for (size_t i = 0; i < n; ++i) {
                    const double x = buf[i * PP + j];
                    if (mean) mean[(m * P + j) * n + i] = x;
                    if (m2) m2[(m * P + j) * n + i] = x * x;
                }
        }
        HIPC(h, hipMemcpy(s1.data(), im.smu, nm * sizeof(double), hipMemcpyDeviceToHost));
        HIPC(h, hipMemcpy(s2.data(), im.smu2, nm * sizeof(double), hipMemcpyDeviceToHost));
        HIPC(h, hipMemcpy(row.data(), im.row, nm * sizeof(int), hipMemcpyDeviceToHost));
        HIPC(h, hipMemcpy(col.data(), im.col, nm * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < nm; ++e) {
            const size_t m = (size_t)col[e] / PP, j = (size_t)col[e] - m * PP, o = (m * P + j) * n + row[e];
            if (mean) mean[o] = s1[e] / cnt;
            if (m2) m2[o] = s2[e] / cnt;
        }
    }
    if (nvar) {
        std::vector<double> sv(ncol);
        std::vector<int> cols(ncol);
        HIPC(h, hipMemcpy(sv.data(), im.snv, ncol * sizeof(double), hipMemcpyDeviceToHost));
        HIPC(h, hipMemcpy(cols.data(), im.cols, ncol * sizeof(int), hipMemcpyDeviceToHost));
        std::fill(nvar, nvar + P * G, 0.0);
        for (size_t c = 0; c < ncol; ++c) {
            const size_t m = (size_t)cols[c] / PP, j = (size_t)cols[c] - m * PP;
            nvar[m * P + j] = sv[c] / cnt;
        }
    }
    return DCFM_OK;
}

}  // extern "C"
