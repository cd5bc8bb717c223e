/*
 * dcfm_mex.c — MATLAB MEX gateway to libdcfm (SURVEY §8(b) callers (1), §8(f) row 1).
 * Build on a host with MATLAB:
 *     mex -R2018a dcfm_mex.c -I<repo>/include -L<pkg dir> -ldcfm
 * (the build container has no MATLAB; tests/test_mex_gateway.py compiles this file against
 * a mock of the mx / mex API and drives it, argument checking on the CPU and a whole chain
 * on the GPU).  Commands:
 *   h = dcfm_mex('create', cfg)           cfg fields n P g K rho burnin mcmc thin as bs df ad1
 *                                         bd1 ad2 bd2 seed device inject asm_batch sigma_m2
 *                                         precision_mean partial_corr corr regression
 *   dcfm_mex('set_data', h, Yd)           Yd n x P x g (dc:49-59 done by the caller)
 *   dcfm_mex('set_data_raw', h, Y0, cols) raw n x p0 data + int64 0-based columns (dc:48-59 on GPU)
 *   dcfm_mex('set_state', h, Lambda, ps, omega, psijh, Plam, X, Z, delta, tauh)
 *   dcfm_mex('init_state', h)             dc:68-87 on the GPU (Philox)
 *   dcfm_mex('set_draws', h, NZ, NX, NL, Gpsi, Gdelta, Gps, first, T)   injected draws
 *                                         (matlab/export_draws.m layout; cfg.inject = 1)
 *   dcfm_mex('run', h, first, count)      dc:90-197
 *   [Lambda, ps, omega, psijh, Plam, X, Z, eta, delta, tauh] = dcfm_mex('get_state', h)
 *   S = dcfm_mex('get_sigma', h)          Sigmaout (dc:194-195), p x p from the handle
 *   M = dcfm_mex('sigma_moment', h, which[, col0, ncols])   which = 'mean' | 'm2' | 'sd': posterior
 *                                         mean, second moment or standard deviation of Sigma's
 *                                         entries ('m2', 'sd' need cfg.sigma_m2 = 1), p x p or
 *                                         the columns col0 .. col0+ncols-1 (0-based), p x ncols
 *   T = dcfm_mex('precision_mean', h[, col0, ncols])   the posterior mean of the precision matrix,
 *                                         (1/effsamp) * sum over the saved samples of inv(Sigma_s) (needs
 *                                         cfg.precision_mean = 1), p x p or the columns col0 .. col0+ncols-1
 *                                         (0-based), p x ncols; Sigmaout's coordinates
 *   R = dcfm_mex('partial_corr', h, which[, col0, ncols])   which = 'mean' | 'm2' | 'sd': posterior mean,
 *                                         second moment or standard deviation of the partial correlations
 *                                         -T_ab / sqrt(T_aa * T_bb), T = inv(Sigma_s), over the saved samples
 *                                         (needs cfg.partial_corr = 1), p x p or the columns col0 ..
 *                                         col0+ncols-1 (0-based), p x ncols; Sigmaout's coordinates
 *   R = dcfm_mex('corr', h, which[, col0, ncols])   which = 'mean' | 'm2' | 'sd': posterior mean, second moment
 *                                         or standard deviation of the correlations S_ab / sqrt(S_aa * S_bb),
 *                                         S = Sigma_s, over the saved samples (needs cfg.corr = 1), p x p or the
 *                                         columns col0 .. col0+ncols-1 (0-based), p x ncols; Sigmaout's coordinates
 *   c = dcfm_mex('communality', h, which) the same three moments of the communalities
 *                                         sum(Lambda_s(a,:).^2) / S_aa (needs cfg.corr = 1), p x 1
 *   Y = dcfm_mex('sigma_apply', h, V)     Y = Sigmaout * V on the device, V p x nv (any nv >= 1), in
 *                                         Sigmaout's permuted, standardised coordinates
 *   [d, V, res] = dcfm_mex('sigma_eigs', h, r[, tol, max_passes, seed])   the r <= 32 largest eigenpairs
 *                                         of Sigmaout (block Krylov on sigma_apply): d r x 1 descending,
 *                                         V p x r orthonormal, res r x 1 = ||Sigmaout v - d v||_2;
 *                                         defaults tol 1e-10, max_passes ceil(p / min(32, p)) + 1, seed 1
 *   [X, relres, iters] = dcfm_mex('sigma_solve', h, B[, tol, max_iter])   X = Sigmaout \ B on the device
 *                                         (conjugate gradients, every column on its own), B p x nv in
 *                                         Sigmaout's coordinates; relres nv x 1 = ||B - Sigmaout X|| / ||B||
 *                                         per column from a real pass, iters nv x 1 the CG steps taken;
 *                                         defaults tol 1e-10, max_iter min(2 p, 1000)
 *   dcfm_mex('set_probes', h, V[, capacity])   record Q(:,:,s) = V' * Sigma_s * V for every saved sample s of
 *                                         later runs, V p x nv (1 <= nv <= 32) in Sigmaout's coordinates;
 *                                         capacity draws are held (default mcmc / thin; 0 turns it off)
 *   Q = dcfm_mex('probe_draws', h)        the recorded draws, nv x nv x S (0 x 0 x 0 with no probes set)
 *   dcfm_mex('set_precision_probes', h, V[, capacity])   record Q(:,:,s) = V' * inv(Sigma_s) * V and
 *                                         logdet(s) = log(det(Sigma_s)) for every saved sample s of later runs,
 *                                         V p x nv (0 <= nv <= 32; p x 0: the log det alone) in Sigmaout's
 *                                         coordinates; capacity as for 'set_probes'; independent of it
 *   [Q, logdet] = dcfm_mex('precision_draws', h)   the recorded draws, nv x nv x S and S x 1 (empty with
 *                                         nothing set)
 *   dcfm_mex('set_loglik', h[, capacity])  record maha(i,s) = y_i' * inv(Sigma_s) * y_i of every row y_i of the
 *                                         standardised data and logdet(s) for every saved sample s of later
 *                                         runs; capacity as for 'set_probes'; independent of both
 *   [maha, logdet] = dcfm_mex('loglik', h)   the recorded draws, n x S and S x 1 (n x 0 and 0 x 1 with nothing
 *                                         set); log N(y_i; 0, Sigma_s) = -(p*log(2*pi) + logdet(s) + maha(i,s))/2
 *   dcfm_mex('set_predict', h, Ynew, observed[, capacity])   predict the unobserved variables of nt new rows
 *                                         (the columns of Ynew, p x nt, 0 <= nt <= 32, Sigmaout's standardised
 *                                         coordinates) from the observed ones (observed p x 1 double, nonzero =
 *                                         observed; entries of Ynew elsewhere are ignored) under every saved sample
 *                                         of later runs; capacity as for 'set_probes'; one rank only
 *   [mean, m2, cvar, maha, logdet] = dcfm_mex('predict', h)   the accumulated prediction: mean and m2 p x nt (the
 *                                         averages of the conditional mean and of its square), cvar p x 1 (the
 *                                         average conditional variance; total variance cvar + m2 - mean.^2), maha
 *                                         nt x S = y_A' * inv(Sigma_AA_s) * y_A and logdet S x 1 (empty with
 *                                         nothing set)
 *   dcfm_mex('set_missing', h, mask[, capacity])   treat entries of the data as missing: mask n x P x g double in
 *                                         Yd's layout, nonzero = missing ([] turns it off); after 'set_data' only;
 *                                         every later iteration redraws them on the device; capacity saved samples
 *                                         are accumulated (default mcmc / thin; 0: draw only); not with 'set_loglik'
 *   [mean, m2, nvar, count] = dcfm_mex('imputed', h)   the accumulated imputation: mean and m2 n x P x g (at a missing
 *                                         entry the averages of eta_i . lambda_j and of its square, at an observed one
 *                                         Yd and Yd.^2), nvar P x g the average 1 / ps_j of the columns with a missing
 *                                         entry (total variance nvar + m2 - mean.^2), count the samples accumulated
 *                                         (count 0: empty arrays)
 *   dcfm_mex('set_regression', h, resp)   regress the variables resp (1-based indices in Sigmaout's coordinates, at most
 *                                         32, distinct; [] turns it off) on all the others under every saved sample
 *                                         of later runs (needs cfg.regression = 1)
 *   [coef, coef_m2, rcov, rcov_m2, r2, r2_m2, count] = dcfm_mex('regression', h)   the accumulated regression: coef
 *                                         and coef_m2 p x q (the averages of the per-sample coefficients
 *                                         Sigma_OO \ Sigma_OR and of their squares; rows resp are 0), rcov and
 *                                         rcov_m2 q x q (the residual covariance), r2 and r2_m2 q x 1, count the samples
 *                                         accumulated (count 0: empty arrays); SD = sqrt(max(0, m2 - mean.^2))
 *   e = dcfm_mex('error', h, U, s, iters)[||S-S0||_F, ||S0||_F, ||S-S0||_2] vs S0 = UU' + diag(s)
 *   dcfm_mex('set_trace', h, cap); T = dcfm_mex('get_trace', h)     chain trace (count x 4)
 *   dcfm_mex('destroy', h)
 * Every array argument is checked (class double, real, element count from the handle's
 * own dimensions) before the library sees its pointer: the library reads and writes at
 * config-derived sizes, so a wrong-sized MATLAB array must never reach it.
 */

#include "mex.h"
#include "dcfm.h"
#include <float.h>
#include <stdint.h>
#include <string.h>

#define NSLOT 64
typedef struct {
    dcfm_handle *h;
    int64_t n, P, g, K;        /* this handle's dimensions (single rank: g_local = g) */
    int64_t mcmc, thin;        /* default capacity of 'set_probes' */
    int64_t nv;                /* width of the probe block the library holds (0: none) */
    int64_t pnv;               /* width of the precision-probe block the library holds */
    int64_t pnt;               /* new rows of the prediction the library holds */
    int64_t rq;                /* responses of the regression the library holds */
} slot;
static slot S[NSLOT];          /* handles live across calls */

static void cleanup(void) {
    for (int i = 0; i < NSLOT; ++i)
        if (S[i].h) { dcfm_destroy(S[i].h); S[i].h = 0; }
}

static double fld(const mxArray *s, const char *f, double dflt) {
    const mxArray *a = mxGetField(s, 0, f);
    if (!a) return dflt;
    if (!mxIsDouble(a) || mxIsComplex(a) || mxGetNumberOfElements(a) != 1)
        mexErrMsgIdAndTxt("dcfm:cfg", "cfg.%s must be a real double scalar", f);
    return mxGetScalar(a);
}
static double scalar(const mxArray *a, const char *what) {
    if (!mxIsDouble(a) || mxIsComplex(a) || mxGetNumberOfElements(a) != 1)
        mexErrMsgIdAndTxt("dcfm:arg", "%s must be a real double scalar", what);
    return mxGetScalar(a);
}
static slot *get(const mxArray *a) {
    const double v = scalar(a, "handle");
    const int i = (int)v;
    if ((double)i != v || i < 0 || i >= NSLOT || !S[i].h) mexErrMsgIdAndTxt("dcfm:handle", "bad handle");
    return &S[i];
}
/* a real double array of exactly `numel` elements; its data pointer */
static double *need(const mxArray *a, int64_t numel, const char *what) {
    if (!mxIsDouble(a) || mxIsComplex(a))
        mexErrMsgIdAndTxt("dcfm:arg", "%s must be a real double array", what);
    if ((int64_t)mxGetNumberOfElements(a) != numel)
        mexErrMsgIdAndTxt("dcfm:arg", "%s must have %lld elements, got %lld", what, (long long)numel,
                          (long long)mxGetNumberOfElements(a));
    return mxGetDoubles(a);
}
static void nargs(int nrhs, int want, const char *cmd) {
    if (nrhs != want) mexErrMsgIdAndTxt("dcfm:nargs", "'%s' takes %d arguments, got %d", cmd, want - 1, nrhs - 1);
}
static void ck(dcfm_handle *h, int rc) {
    if (rc != DCFM_OK) mexErrMsgIdAndTxt("dcfm:call", "%s", dcfm_last_error(h));
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    char cmd[32];
    mexAtExit(cleanup);
    if (nrhs < 1 || !mxIsChar(prhs[0]) || mxGetString(prhs[0], cmd, sizeof cmd) != 0)
        mexErrMsgIdAndTxt("dcfm:cmd", "first argument must be a command string");
    if (!strcmp(cmd, "create")) {
        nargs(nrhs, 2, cmd);
        const mxArray *s = prhs[1];
        if (!mxIsStruct(s)) mexErrMsgIdAndTxt("dcfm:cfg", "cfg must be a struct");
        dcfm_config c;
        memset(&c, 0, sizeof c);
        c.n = (int32_t)fld(s, "n", 0);  c.P = (int32_t)fld(s, "P", 0);  c.g = (int32_t)fld(s, "g", 0);
        c.K = (int32_t)fld(s, "K", 0);  c.rho = fld(s, "rho", 0);
        c.burnin = (int64_t)fld(s, "burnin", 0); c.mcmc = (int64_t)fld(s, "mcmc", 0);
        c.thin = (int64_t)fld(s, "thin", 1);
        c.as_ = fld(s, "as", 1); c.bs = fld(s, "bs", 0.3); c.df = fld(s, "df", 3);
        c.ad1 = fld(s, "ad1", 2); c.bd1 = fld(s, "bd1", 1); c.ad2 = fld(s, "ad2", 2); c.bd2 = fld(s, "bd2", 1);
        c.seed = (uint64_t)fld(s, "seed", 0); c.nranks = 1; c.device = (int32_t)fld(s, "device", 0);
        c.flags = fld(s, "inject", 0) != 0 ? DCFM_FLAG_INJECT_DRAWS : 0u;
        if (fld(s, "sigma_m2", 0) != 0) c.flags |= DCFM_FLAG_SIGMA_M2;
        if (fld(s, "precision_mean", 0) != 0) c.flags |= DCFM_FLAG_PRECISION_MEAN;
        if (fld(s, "partial_corr", 0) != 0) c.flags |= DCFM_FLAG_PARTIAL_CORR;
        if (fld(s, "corr", 0) != 0) c.flags |= DCFM_FLAG_CORR;
        if (fld(s, "regression", 0) != 0) c.flags |= DCFM_FLAG_REGRESSION;
        c.asm_batch = (int32_t)fld(s, "asm_batch", 0);
        int i = 0;
        while (i < NSLOT && S[i].h) ++i;
        if (i == NSLOT) mexErrMsgIdAndTxt("dcfm:handle", "too many handles");
        if (dcfm_create(&c, &S[i].h) != DCFM_OK) {
            S[i].h = 0;
            mexErrMsgIdAndTxt("dcfm:create", "%s", dcfm_last_error(NULL));
        }
        S[i].n = c.n; S[i].P = c.P; S[i].g = c.g; S[i].K = c.K;
        S[i].mcmc = c.mcmc; S[i].thin = c.thin; S[i].nv = 0; S[i].pnv = 0; S[i].pnt = 0; S[i].rq = 0;
        mexLock();
        plhs[0] = mxCreateDoubleScalar(i);
    } else if (!strcmp(cmd, "set_data")) {
        nargs(nrhs, 3, cmd);
        slot *t = get(prhs[1]);
        ck(t->h, dcfm_set_data(t->h, need(prhs[2], t->n * t->P * t->g, "Yd (n x P x g)")));
    } else if (!strcmp(cmd, "set_state")) {          /* Lambda ps omega psi Plam X Z delta tauh */
        nargs(nrhs, 11, cmd);
        slot *t = get(prhs[1]);
        const int64_t PKg = t->P * t->K * t->g, Pg = t->P * t->g, nK = t->n * t->K, Kg = t->K * t->g;
        dcfm_state_view v;
        memset(&v, 0, sizeof v);
        v.Lambda = need(prhs[2], PKg, "Lambda (P x K x g)");
        v.ps = need(prhs[3], Pg, "ps (P x 1 x g)");
        v.omega = need(prhs[4], Pg, "omega (P x g)");
        v.psi = need(prhs[5], PKg, "psijh (P x K x g)");
        v.Plam = need(prhs[6], PKg, "Plam (P x K x g)");
        v.X = need(prhs[7], nK, "X (n x K)");
        v.Z = need(prhs[8], nK * t->g, "Z (n x K x g)");
        v.delta = need(prhs[9], Kg, "delta (K x 1 x g)");
        v.tauh = need(prhs[10], Kg, "tauh (K x 1 x g)");
        ck(t->h, dcfm_set_state(t->h, &v));
    } else if (!strcmp(cmd, "get_state")) {
        nargs(nrhs, 2, cmd);
        slot *t = get(prhs[1]);
        const mwSize P = (mwSize)t->P, K = (mwSize)t->K, g = (mwSize)t->g, n = (mwSize)t->n;
        const mwSize dPKg[3] = {P, K, g}, dP1g[3] = {P, 1, g}, dnKg[3] = {n, K, g}, dK1g[3] = {K, 1, g};
        mxArray *o[10];
        o[0] = mxCreateNumericArray(3, dPKg, mxDOUBLE_CLASS, mxREAL);   /* Lambda */
        o[1] = mxCreateNumericArray(3, dP1g, mxDOUBLE_CLASS, mxREAL);   /* ps */
        o[2] = mxCreateDoubleMatrix(P, g, mxREAL);                      /* omega */
        o[3] = mxCreateNumericArray(3, dPKg, mxDOUBLE_CLASS, mxREAL);   /* psijh */
        o[4] = mxCreateNumericArray(3, dPKg, mxDOUBLE_CLASS, mxREAL);   /* Plam */
        o[5] = mxCreateDoubleMatrix(n, K, mxREAL);                      /* X */
        o[6] = mxCreateNumericArray(3, dnKg, mxDOUBLE_CLASS, mxREAL);   /* Z */
        o[7] = mxCreateNumericArray(3, dnKg, mxDOUBLE_CLASS, mxREAL);   /* eta */
        o[8] = mxCreateNumericArray(3, dK1g, mxDOUBLE_CLASS, mxREAL);   /* delta */
        o[9] = mxCreateNumericArray(3, dK1g, mxDOUBLE_CLASS, mxREAL);   /* tauh */
        dcfm_state_view v;
        v.Lambda = mxGetDoubles(o[0]); v.ps = mxGetDoubles(o[1]); v.omega = mxGetDoubles(o[2]);
        v.psi = mxGetDoubles(o[3]); v.Plam = mxGetDoubles(o[4]); v.X = mxGetDoubles(o[5]);
        v.Z = mxGetDoubles(o[6]); v.eta = mxGetDoubles(o[7]); v.delta = mxGetDoubles(o[8]);
        v.tauh = mxGetDoubles(o[9]);
        ck(t->h, dcfm_get_state(t->h, &v));
        for (int q = 0; q < 10; ++q) {
            if (q < (nlhs < 1 ? 1 : nlhs)) plhs[q] = o[q];
            else mxDestroyArray(o[q]);
        }
    } else if (!strcmp(cmd, "set_data_raw")) {       /* Y0 (n x p0 double), cols (int64, 0-based) */
        nargs(nrhs, 4, cmd);
        slot *t = get(prhs[1]);
        const mxArray *Y = prhs[2], *cols = prhs[3];
        if (!mxIsDouble(Y) || mxIsComplex(Y) || (int64_t)mxGetM(Y) != t->n)
            mexErrMsgIdAndTxt("dcfm:arg", "Y0 must be a real double n x p0 matrix (n = %lld)", (long long)t->n);
        const int64_t p0 = (int64_t)mxGetN(Y);
        if (!mxIsInt64(cols) || (int64_t)mxGetNumberOfElements(cols) != t->P * t->g)
            mexErrMsgIdAndTxt("dcfm:cols", "cols must be int64 with P*g = %lld elements", (long long)(t->P * t->g));
        const int64_t *cv = (const int64_t *)mxGetInt64s(cols);
        for (int64_t e = 0; e < t->P * t->g; ++e)
            if (cv[e] < 0 || cv[e] >= p0) mexErrMsgIdAndTxt("dcfm:cols", "cols(%lld) = %lld outside 0..p0-1",
                                                             (long long)(e + 1), (long long)cv[e]);
        ck(t->h, dcfm_set_data_raw(t->h, mxGetDoubles(Y), p0, cv, NULL, NULL));
    } else if (!strcmp(cmd, "init_state")) {
        nargs(nrhs, 2, cmd);
        slot *t = get(prhs[1]);
        ck(t->h, dcfm_init_state(t->h));
    } else if (!strcmp(cmd, "set_draws")) {          /* NZ NX NL Gpsi Gdelta Gps first T */
        nargs(nrhs, 10, cmd);
        slot *t = get(prhs[1]);
        const double first = scalar(prhs[8], "first"), T = scalar(prhs[9], "T");
        if (T < 1 || T != (double)(int64_t)T || first != (double)(int64_t)first)
            mexErrMsgIdAndTxt("dcfm:arg", "first and T must be integers, T >= 1");
        const int64_t nT = (int64_t)T;
        dcfm_draws_view v;
        v.NZ = need(prhs[2], t->K * t->n * t->g * nT, "NZ (K x n x g x T)");
        v.NX = need(prhs[3], t->K * t->n * nT, "NX (K x n x T)");
        v.NL = need(prhs[4], t->K * t->P * t->g * nT, "NL (K x P x g x T)");
        v.Gpsi = need(prhs[5], t->P * t->K * t->g * nT, "Gpsi (P x K x g x T)");
        v.Gdelta = need(prhs[6], t->K * t->g * nT, "Gdelta (K x g x T)");
        v.Gps = need(prhs[7], t->P * t->g * nT, "Gps (P x g x T)");
        ck(t->h, dcfm_set_draws(t->h, &v, (int64_t)first, nT));
    } else if (!strcmp(cmd, "error")) {              /* e = dcfm_mex('error', h, U, s, iters) */
        nargs(nrhs, 5, cmd);
        slot *t = get(prhs[1]);
        const int64_t p = t->P * t->g;
        const mxArray *U = prhs[2];
        if (!mxIsDouble(U) || mxIsComplex(U) || (int64_t)mxGetM(U) != p || mxGetN(U) < 1 || mxGetN(U) > 32)
            mexErrMsgIdAndTxt("dcfm:arg", "U must be a real double p x r matrix, p = %lld, 1 <= r <= 32", (long long)p);
        const double *sv = need(prhs[3], p, "s (p x 1)");
        const double it = scalar(prhs[4], "iters");
        if (it < 0 || it != (double)(int32_t)it) mexErrMsgIdAndTxt("dcfm:arg", "iters must be a non-negative integer");
        plhs[0] = mxCreateDoubleMatrix(1, 3, mxREAL);
        ck(t->h, dcfm_sigma_error(t->h, mxGetDoubles(U), (int32_t)mxGetN(U), sv, (int32_t)it, 1,
                                  mxGetDoubles(plhs[0])));
    } else if (!strcmp(cmd, "set_trace")) {
        nargs(nrhs, 3, cmd);
        slot *t = get(prhs[1]);
        const double cap = scalar(prhs[2], "cap");
        if (cap < 0) mexErrMsgIdAndTxt("dcfm:arg", "cap must be >= 0");
        ck(t->h, dcfm_set_trace(t->h, (int64_t)cap));
    } else if (!strcmp(cmd, "get_trace")) {          /* count x 4, MATLAB column-major */
        nargs(nrhs, 2, cmd);
        slot *t = get(prhs[1]);
        int64_t cnt = 0;
        ck(t->h, dcfm_get_trace(t->h, NULL, &cnt));
        double *rows = (double *)mxMalloc((size_t)(cnt > 0 ? cnt : 1) * 4 * sizeof(double));
        ck(t->h, dcfm_get_trace(t->h, rows, &cnt));
        plhs[0] = mxCreateDoubleMatrix((mwSize)cnt, 4, mxREAL);
        double *o = mxGetDoubles(plhs[0]);
        for (int64_t r = 0; r < cnt; ++r)
            for (int q = 0; q < 4; ++q) o[r + cnt * q] = rows[r * 4 + q];
        mxFree(rows);
    } else if (!strcmp(cmd, "run")) {
        nargs(nrhs, 4, cmd);
        slot *t = get(prhs[1]);
        const double first = scalar(prhs[2], "first"), count = scalar(prhs[3], "count");
        if (first < 1 || count < 0 || first != (double)(int64_t)first || count != (double)(int64_t)count)
            mexErrMsgIdAndTxt("dcfm:arg", "first >= 1 and count >= 0 must be integers");
        ck(t->h, dcfm_run(t->h, (int64_t)first, (int64_t)count));
    } else if (!strcmp(cmd, "get_sigma")) {          /* Sigmaout = dcfm_mex('get_sigma', h) */
        if (nrhs != 2 && nrhs != 3) nargs(nrhs, 2, cmd);
        slot *t = get(prhs[1]);
        const int64_t p = t->P * t->g;               /* the size the library writes */
        if (nrhs == 3 && scalar(prhs[2], "p") != (double)p)
            mexErrMsgIdAndTxt("dcfm:arg", "p = %g does not match the handle's P*g = %lld", mxGetScalar(prhs[2]),
                              (long long)p);
        plhs[0] = mxCreateDoubleMatrix((mwSize)p, (mwSize)p, mxREAL);
        ck(t->h, dcfm_get_sigma(t->h, mxGetDoubles(plhs[0])));
    } else if (!strcmp(cmd, "sigma_moment") || !strcmp(cmd, "partial_corr") || !strcmp(cmd, "corr") ||
               !strcmp(cmd, "communality")) {
        /* M = dcfm_mex('sigma_moment', h, which[, col0, ncols]), R = dcfm_mex('partial_corr' | 'corr', h, which[, col0,
         * ncols]), c = dcfm_mex('communality', h, which) */
        const int vec = !strcmp(cmd, "communality");   /* a p-vector: no column range */
        if (vec && nrhs != 3) mexErrMsgIdAndTxt("dcfm:nargs", "'%s' takes 2 arguments, got %d", cmd, nrhs - 1);
        if (nrhs != 3 && nrhs != 5)
            mexErrMsgIdAndTxt("dcfm:nargs", "'%s' takes 2 or 4 arguments, got %d", cmd, nrhs - 1);
        /* the arguments that need no handle first: a malformed call never reaches the library */
        char wn[8];
        int32_t which = -1;
        if (mxIsChar(prhs[2]) && mxGetString(prhs[2], wn, sizeof wn) == 0) {
            if (!strcmp(wn, "mean")) which = DCFM_SIGMA_MEAN;
            else if (!strcmp(wn, "m2")) which = DCFM_SIGMA_M2;
            else if (!strcmp(wn, "sd")) which = DCFM_SIGMA_SD;
        }
        if (which < 0) mexErrMsgIdAndTxt("dcfm:arg", "which must be 'mean', 'm2' or 'sd'");
        double c0 = 0, nc = -1;                      /* 0-based first column and count; default: all */
        if (nrhs == 5) {
            c0 = scalar(prhs[3], "col0");
            nc = scalar(prhs[4], "ncols");
            if (c0 < 0 || nc < 0 || c0 != (double)(int64_t)c0 || nc != (double)(int64_t)nc)
                mexErrMsgIdAndTxt("dcfm:arg", "col0 and ncols must be non-negative integers");
        }
        slot *t = get(prhs[1]);
        const int64_t p = t->P * t->g;               /* the size the library writes */
        if (nc < 0) nc = vec ? 1.0 : (double)p;
        if (!vec && c0 + nc > (double)p)
            mexErrMsgIdAndTxt("dcfm:arg", "columns [%g, %g) outside 0..p = %lld", c0, c0 + nc, (long long)p);
        plhs[0] = mxCreateDoubleMatrix((mwSize)p, (mwSize)nc, mxREAL);
        if (vec)
            ck(t->h, dcfm_get_communality(t->h, which, mxGetDoubles(plhs[0])));
        else if (!strcmp(cmd, "corr"))
            ck(t->h, dcfm_get_corr_cols(t->h, which, (int64_t)c0, (int64_t)nc, mxGetDoubles(plhs[0])));
        else if (!strcmp(cmd, "partial_corr"))
            ck(t->h, dcfm_get_partial_corr_cols(t->h, which, (int64_t)c0, (int64_t)nc, mxGetDoubles(plhs[0])));
        else
            ck(t->h, dcfm_get_sigma_moment_cols(t->h, which, (int64_t)c0, (int64_t)nc, mxGetDoubles(plhs[0])));
    } else if (!strcmp(cmd, "precision_mean")) {     /* T = dcfm_mex('precision_mean', h[, col0, ncols]) */
        if (nrhs != 2 && nrhs != 4)
            mexErrMsgIdAndTxt("dcfm:nargs", "'%s' takes 1 or 3 arguments, got %d", cmd, nrhs - 1);
        double c0 = 0, nc = -1;                      /* checked as 'sigma_moment' checks its range */
        if (nrhs == 4) {
            c0 = scalar(prhs[2], "col0");
            nc = scalar(prhs[3], "ncols");
            if (c0 < 0 || nc < 0 || c0 != (double)(int64_t)c0 || nc != (double)(int64_t)nc)
                mexErrMsgIdAndTxt("dcfm:arg", "col0 and ncols must be non-negative integers");
        }
        slot *t = get(prhs[1]);
        const int64_t p = t->P * t->g;               /* the size the library writes */
        if (nc < 0) nc = (double)p;
        if (c0 + nc > (double)p)
            mexErrMsgIdAndTxt("dcfm:arg", "columns [%g, %g) outside 0..p = %lld", c0, c0 + nc, (long long)p);
        plhs[0] = mxCreateDoubleMatrix((mwSize)p, (mwSize)nc, mxREAL);
        ck(t->h, dcfm_get_precision_mean_cols(t->h, (int64_t)c0, (int64_t)nc, mxGetDoubles(plhs[0])));
    } else if (!strcmp(cmd, "sigma_apply")) {        /* Y = dcfm_mex('sigma_apply', h, V) */
        nargs(nrhs, 3, cmd);
        slot *t = get(prhs[1]);
        const int64_t p = t->P * t->g;               /* the row count the library reads and writes */
        const mxArray *V = prhs[2];
        if (!mxIsDouble(V) || mxIsComplex(V) || (int64_t)mxGetM(V) != p || mxGetN(V) < 1 || mxGetN(V) > 2147483647 ||
            (int64_t)mxGetNumberOfElements(V) != p * (int64_t)mxGetN(V))
            mexErrMsgIdAndTxt("dcfm:arg", "V must be a real double p x nv matrix, p = %lld, nv >= 1", (long long)p);
        plhs[0] = mxCreateDoubleMatrix((mwSize)p, mxGetN(V), mxREAL);
        ck(t->h, dcfm_sigma_apply(t->h, mxGetDoubles(V), (int32_t)mxGetN(V), mxGetDoubles(plhs[0]), NULL));
    } else if (!strcmp(cmd, "sigma_eigs")) {         /* [d, V, res] = dcfm_mex('sigma_eigs', h, r[, tol, max_passes, seed]) */
        if (nrhs < 3 || nrhs > 6)
            mexErrMsgIdAndTxt("dcfm:nargs", "'%s' takes 2 to 5 arguments, got %d", cmd, nrhs - 1);
        /* the arguments that need no handle first: a malformed call never reaches the library */
        const double rr = scalar(prhs[2], "r");
        const double tol = nrhs > 3 ? scalar(prhs[3], "tol") : 1e-10;
        const double mp = nrhs > 4 ? scalar(prhs[4], "max_passes") : 0;
        const double sd = nrhs > 5 ? scalar(prhs[5], "seed") : 1;
        if (rr < 1 || rr > 32 || rr != (double)(int32_t)rr) mexErrMsgIdAndTxt("dcfm:arg", "r must be an integer in 1..32");
        if (!(tol > 0)) mexErrMsgIdAndTxt("dcfm:arg", "tol must be > 0");
        if (nrhs > 4 && (mp < 1 || mp > 2147483647.0 || mp != (double)(int32_t)mp))
            mexErrMsgIdAndTxt("dcfm:arg", "max_passes must be a positive integer");
        if (sd < 0 || sd > 9007199254740992.0 || sd != (double)(uint64_t)sd)
            mexErrMsgIdAndTxt("dcfm:arg", "seed must be a non-negative integer");
        slot *t = get(prhs[1]);
        const int64_t p = t->P * t->g, b = p < 32 ? p : 32;
        if (rr > (double)p) mexErrMsgIdAndTxt("dcfm:arg", "r = %g exceeds p = %lld", rr, (long long)p);
        const int32_t r = (int32_t)rr, passes = nrhs > 4 ? (int32_t)mp : (int32_t)((p + b - 1) / b + 1);
        mxArray *o[3];
        o[0] = mxCreateDoubleMatrix((mwSize)r, 1, mxREAL);
        o[1] = mxCreateDoubleMatrix((mwSize)p, (mwSize)r, mxREAL);
        o[2] = mxCreateDoubleMatrix((mwSize)r, 1, mxREAL);
        ck(t->h, dcfm_sigma_eigs(t->h, r, tol, passes, (uint64_t)sd, mxGetDoubles(o[0]), mxGetDoubles(o[1]),
                                 mxGetDoubles(o[2]), NULL));
        for (int q = 0; q < 3; ++q) {
            if (q < (nlhs < 1 ? 1 : nlhs)) plhs[q] = o[q];
            else mxDestroyArray(o[q]);
        }
    } else if (!strcmp(cmd, "sigma_solve")) {        /* [X, relres, iters] = dcfm_mex('sigma_solve', h, B[, tol, max_iter]) */
        if (nrhs < 3 || nrhs > 5)
            mexErrMsgIdAndTxt("dcfm:nargs", "'%s' takes 2 to 4 arguments, got %d", cmd, nrhs - 1);
        /* the arguments that need no handle first: a malformed call never reaches the library */
        const double tol = nrhs > 3 ? scalar(prhs[3], "tol") : 1e-10;
        const double mi = nrhs > 4 ? scalar(prhs[4], "max_iter") : 0;
        if (!(tol > 0) || tol > DBL_MAX) mexErrMsgIdAndTxt("dcfm:arg", "tol must be a positive finite number");
        if (nrhs > 4 && (mi < 1 || mi > 2147483647.0 || mi != (double)(int32_t)mi))
            mexErrMsgIdAndTxt("dcfm:arg", "max_iter must be a positive integer");
        slot *t = get(prhs[1]);
        const int64_t p = t->P * t->g;               /* the row count the library reads and writes */
        const mxArray *B = prhs[2];
        if (!mxIsDouble(B) || mxIsComplex(B) || (int64_t)mxGetM(B) != p || mxGetN(B) < 1 || mxGetN(B) > 2147483647 ||
            (int64_t)mxGetNumberOfElements(B) != p * (int64_t)mxGetN(B))
            mexErrMsgIdAndTxt("dcfm:arg", "B must be a real double p x nv matrix, p = %lld, nv >= 1", (long long)p);
        const int32_t nv = (int32_t)mxGetN(B), max_iter = nrhs > 4 ? (int32_t)mi : (int32_t)(2 * p < 1000 ? 2 * p : 1000);
        mxArray *o[3];
        o[0] = mxCreateDoubleMatrix((mwSize)p, (mwSize)nv, mxREAL);
        o[1] = mxCreateDoubleMatrix((mwSize)nv, 1, mxREAL);
        o[2] = mxCreateDoubleMatrix((mwSize)nv, 1, mxREAL);
        /* the library's int32 steps land in the front half of o[2]'s own storage (nothing to free if the
         * call fails) and are widened in place from the back */
        double *itd = mxGetDoubles(o[2]);
        ck(t->h, dcfm_sigma_solve(t->h, mxGetDoubles(B), nv, tol, max_iter, mxGetDoubles(o[0]), mxGetDoubles(o[1]),
                                  (int32_t *)itd, NULL, NULL));
        for (int32_t c = nv - 1; c >= 0; --c) {
            int32_t v;
            memcpy(&v, (const char *)itd + (size_t)c * sizeof v, sizeof v);
            itd[c] = (double)v;
        }
        for (int q = 0; q < 3; ++q) {
            if (q < (nlhs < 1 ? 1 : nlhs)) plhs[q] = o[q];
            else mxDestroyArray(o[q]);
        }
    } else if (!strcmp(cmd, "set_probes")) {         /* dcfm_mex('set_probes', h, V[, capacity]) */
        if (nrhs != 3 && nrhs != 4)
            mexErrMsgIdAndTxt("dcfm:nargs", "'%s' takes 2 or 3 arguments, got %d", cmd, nrhs - 1);
        /* the argument that needs no handle first: a malformed call never reaches the library */
        const double cap = nrhs > 3 ? scalar(prhs[3], "capacity") : -1;
        if (nrhs > 3 && (cap < 0 || cap > 9007199254740992.0 || cap != (double)(int64_t)cap))
            mexErrMsgIdAndTxt("dcfm:arg", "capacity must be a non-negative integer");
        slot *t = get(prhs[1]);
        const int64_t p = t->P * t->g;               /* the row count the library reads */
        const int64_t capacity = nrhs > 3 ? (int64_t)cap : (t->thin > 0 ? t->mcmc / t->thin : 0);
        const mxArray *V = prhs[2];
        if (capacity > 0 && (!mxIsDouble(V) || mxIsComplex(V) || (int64_t)mxGetM(V) != p || mxGetN(V) < 1 ||
                             mxGetN(V) > 32 || (int64_t)mxGetNumberOfElements(V) != p * (int64_t)mxGetN(V)))
            mexErrMsgIdAndTxt("dcfm:arg", "V must be a real double p x nv matrix, p = %lld, 1 <= nv <= 32", (long long)p);
        if (capacity > 0) {
            ck(t->h, dcfm_set_probes(t->h, mxGetDoubles(V), (int32_t)mxGetN(V), capacity));
            t->nv = (int64_t)mxGetN(V);
        } else {
            ck(t->h, dcfm_set_probes(t->h, NULL, 0, 0));
            t->nv = 0;
        }
    } else if (!strcmp(cmd, "probe_draws")) {        /* Q = dcfm_mex('probe_draws', h), nv x nv x S */
        nargs(nrhs, 2, cmd);
        slot *t = get(prhs[1]);
        int64_t cnt = 0;
        ck(t->h, dcfm_get_probe_draws(t->h, NULL, &cnt));
        const mwSize nv = (mwSize)(cnt > 0 ? t->nv : 0), dq[3] = {nv, nv, (mwSize)cnt};
        plhs[0] = mxCreateNumericArray(3, dq, mxDOUBLE_CLASS, mxREAL);   /* the size the library writes */
        if (cnt > 0) ck(t->h, dcfm_get_probe_draws(t->h, mxGetDoubles(plhs[0]), &cnt));
    } else if (!strcmp(cmd, "set_precision_probes")) {   /* dcfm_mex('set_precision_probes', h, V[, capacity]) */
        if (nrhs != 3 && nrhs != 4)
            mexErrMsgIdAndTxt("dcfm:nargs", "'%s' takes 2 or 3 arguments, got %d", cmd, nrhs - 1);
        /* the argument that needs no handle first: a malformed call never reaches the library */
        const double cap = nrhs > 3 ? scalar(prhs[3], "capacity") : -1;
        if (nrhs > 3 && (cap < 0 || cap > 9007199254740992.0 || cap != (double)(int64_t)cap))
            mexErrMsgIdAndTxt("dcfm:arg", "capacity must be a non-negative integer");
        slot *t = get(prhs[1]);
        const int64_t p = t->P * t->g;               /* the row count the library reads */
        const int64_t capacity = nrhs > 3 ? (int64_t)cap : (t->thin > 0 ? t->mcmc / t->thin : 0);
        const mxArray *V = prhs[2];
        if (capacity > 0 && (!mxIsDouble(V) || mxIsComplex(V) || (int64_t)mxGetM(V) != p || mxGetN(V) > 32 ||
                             (int64_t)mxGetNumberOfElements(V) != p * (int64_t)mxGetN(V)))
            mexErrMsgIdAndTxt("dcfm:arg", "V must be a real double p x nv matrix, p = %lld, 0 <= nv <= 32", (long long)p);
        if (capacity > 0) {
            const int32_t nv = (int32_t)mxGetN(V);
            ck(t->h, dcfm_set_precision_probes(t->h, nv > 0 ? mxGetDoubles(V) : NULL, nv, capacity));
            t->pnv = nv;
        } else {
            ck(t->h, dcfm_set_precision_probes(t->h, NULL, 0, 0));
            t->pnv = 0;
        }
    } else if (!strcmp(cmd, "precision_draws")) {    /* [Q, logdet] = dcfm_mex('precision_draws', h) */
        nargs(nrhs, 2, cmd);
        slot *t = get(prhs[1]);
        int64_t cnt = 0;
        ck(t->h, dcfm_get_precision_draws(t->h, NULL, NULL, &cnt));
        const mwSize nv = (mwSize)(cnt > 0 ? t->pnv : 0), dq[3] = {nv, nv, (mwSize)cnt};
        mxArray *Q = mxCreateNumericArray(3, dq, mxDOUBLE_CLASS, mxREAL);   /* the sizes the library writes */
        mxArray *ld = mxCreateDoubleMatrix((mwSize)cnt, 1, mxREAL);
        if (cnt > 0) ck(t->h, dcfm_get_precision_draws(t->h, nv > 0 ? mxGetDoubles(Q) : NULL, mxGetDoubles(ld), &cnt));
        plhs[0] = Q;
        if (nlhs > 1) plhs[1] = ld;
        else mxDestroyArray(ld);
    } else if (!strcmp(cmd, "set_loglik")) {         /* dcfm_mex('set_loglik', h[, capacity]) */
        if (nrhs != 2 && nrhs != 3)
            mexErrMsgIdAndTxt("dcfm:nargs", "'%s' takes 1 or 2 arguments, got %d", cmd, nrhs - 1);
        /* the argument that needs no handle first: a malformed call never reaches the library */
        const double cap = nrhs > 2 ? scalar(prhs[2], "capacity") : -1;
        if (nrhs > 2 && (cap < 0 || cap > 9007199254740992.0 || cap != (double)(int64_t)cap))
            mexErrMsgIdAndTxt("dcfm:arg", "capacity must be a non-negative integer");
        slot *t = get(prhs[1]);
        ck(t->h, dcfm_set_loglik(t->h, nrhs > 2 ? (int64_t)cap : (t->thin > 0 ? t->mcmc / t->thin : 0)));
    } else if (!strcmp(cmd, "loglik")) {             /* [maha, logdet] = dcfm_mex('loglik', h) */
        nargs(nrhs, 2, cmd);
        slot *t = get(prhs[1]);
        int64_t cnt = 0;
        ck(t->h, dcfm_get_loglik(t->h, NULL, NULL, &cnt));
        mxArray *q = mxCreateDoubleMatrix((mwSize)t->n, (mwSize)cnt, mxREAL);   /* the sizes the library writes */
        mxArray *ld = mxCreateDoubleMatrix((mwSize)cnt, 1, mxREAL);
        if (cnt > 0) ck(t->h, dcfm_get_loglik(t->h, mxGetDoubles(q), mxGetDoubles(ld), &cnt));
        plhs[0] = q;
        if (nlhs > 1) plhs[1] = ld;
        else mxDestroyArray(ld);
    } else if (!strcmp(cmd, "set_predict")) {        /* dcfm_mex('set_predict', h, Ynew, observed[, capacity]) */
        if (nrhs != 4 && nrhs != 5)
            mexErrMsgIdAndTxt("dcfm:nargs", "'%s' takes 3 or 4 arguments, got %d", cmd, nrhs - 1);
        /* the argument that needs no handle first: a malformed call never reaches the library */
        const double cap = nrhs > 4 ? scalar(prhs[4], "capacity") : -1;
        if (nrhs > 4 && (cap < 0 || cap > 9007199254740992.0 || cap != (double)(int64_t)cap))
            mexErrMsgIdAndTxt("dcfm:arg", "capacity must be a non-negative integer");
        slot *t = get(prhs[1]);
        const int64_t p = t->P * t->g;               /* the row count the library reads */
        const int64_t capacity = nrhs > 4 ? (int64_t)cap : (t->thin > 0 ? t->mcmc / t->thin : 0);
        const mxArray *Y = prhs[2], *ob = prhs[3];
        if (capacity > 0 && (!mxIsDouble(Y) || mxIsComplex(Y) || (int64_t)mxGetM(Y) != p || mxGetN(Y) > 32 ||
                             (int64_t)mxGetNumberOfElements(Y) != p * (int64_t)mxGetN(Y)))
            mexErrMsgIdAndTxt("dcfm:arg", "Ynew must be a real double p x nt matrix, p = %lld, 0 <= nt <= 32", (long long)p);
        if (capacity > 0 && (!mxIsDouble(ob) || mxIsComplex(ob) || (int64_t)mxGetNumberOfElements(ob) != p))
            mexErrMsgIdAndTxt("dcfm:arg", "observed must be a real double vector of p = %lld elements", (long long)p);
        if (capacity > 0) {
            const int32_t nt = (int32_t)mxGetN(Y);
            uint8_t *mask = (uint8_t *)mxMalloc((mwSize)p);
            const double *od = mxGetDoubles(ob);
            for (int64_t j = 0; j < p; ++j) mask[j] = od[j] != 0.0;
            const int rc = dcfm_set_predict(t->h, nt > 0 ? mxGetDoubles(Y) : NULL, mask, nt, capacity);
            mxFree(mask);
            ck(t->h, rc);
            t->pnt = nt;
        } else {
            ck(t->h, dcfm_set_predict(t->h, NULL, NULL, 0, 0));
            t->pnt = 0;
        }
    } else if (!strcmp(cmd, "predict")) {            /* [mean, m2, cvar, maha, logdet] = dcfm_mex('predict', h) */
        nargs(nrhs, 2, cmd);
        slot *t = get(prhs[1]);
        int64_t cnt = 0;
        ck(t->h, dcfm_get_predict(t->h, NULL, NULL, NULL, NULL, NULL, &cnt));
        const mwSize p = (mwSize)(t->P * t->g), nt = (mwSize)(cnt > 0 ? t->pnt : 0);
        mxArray *o[5];                               /* the sizes the library writes */
        o[0] = mxCreateDoubleMatrix(p, nt, mxREAL);
        o[1] = mxCreateDoubleMatrix(p, nt, mxREAL);
        o[2] = mxCreateDoubleMatrix(cnt > 0 ? p : 0, cnt > 0 ? 1 : 0, mxREAL);
        o[3] = mxCreateDoubleMatrix(nt, (mwSize)cnt, mxREAL);
        o[4] = mxCreateDoubleMatrix((mwSize)cnt, 1, mxREAL);
        if (cnt > 0)
            ck(t->h, dcfm_get_predict(t->h, nt > 0 ? mxGetDoubles(o[0]) : NULL, nt > 0 ? mxGetDoubles(o[1]) : NULL,
                                      mxGetDoubles(o[2]), nt > 0 ? mxGetDoubles(o[3]) : NULL, mxGetDoubles(o[4]), &cnt));
        for (int i = 0; i < 5; ++i)
            if (i == 0 || i < nlhs) plhs[i] = o[i];
            else mxDestroyArray(o[i]);
    } else if (!strcmp(cmd, "set_missing")) {        /* dcfm_mex('set_missing', h, mask[, capacity]) */
        if (nrhs != 3 && nrhs != 4)
            mexErrMsgIdAndTxt("dcfm:nargs", "'%s' takes 2 or 3 arguments, got %d", cmd, nrhs - 1);
        /* the argument that needs no handle first: a malformed call never reaches the library */
        const double cap = nrhs > 3 ? scalar(prhs[3], "capacity") : -1;
        if (nrhs > 3 && (cap < 0 || cap > 9007199254740992.0 || cap != (double)(int64_t)cap))
            mexErrMsgIdAndTxt("dcfm:arg", "capacity must be a non-negative integer");
        slot *t = get(prhs[1]);
        const int64_t numel = t->n * t->P * t->g;    /* the bytes the library reads */
        const int64_t capacity = nrhs > 3 ? (int64_t)cap : (t->thin > 0 ? t->mcmc / t->thin : 0);
        const mxArray *mk = prhs[2];
        if (!mxIsDouble(mk) || mxIsComplex(mk) ||
            (mxGetNumberOfElements(mk) != 0 && (int64_t)mxGetNumberOfElements(mk) != numel))
            mexErrMsgIdAndTxt("dcfm:arg", "mask must be a real double n x P x g array of %lld elements, or empty",
                              (long long)numel);
        if (mxGetNumberOfElements(mk) == 0) {        /* []: off */
            ck(t->h, dcfm_set_missing(t->h, NULL, capacity));
        } else {
            uint8_t *mask = (uint8_t *)mxMalloc((mwSize)numel);
            const double *md = mxGetDoubles(mk);
            for (int64_t q = 0; q < numel; ++q) mask[q] = md[q] != 0.0;
            const int rc = dcfm_set_missing(t->h, mask, capacity);
            mxFree(mask);
            ck(t->h, rc);
        }
    } else if (!strcmp(cmd, "imputed")) {            /* [mean, m2, nvar, count] = dcfm_mex('imputed', h) */
        nargs(nrhs, 2, cmd);
        slot *t = get(prhs[1]);
        int64_t cnt = 0;
        ck(t->h, dcfm_get_imputed(t->h, NULL, NULL, NULL, &cnt));
        const mwSize on = cnt > 0 ? 1 : 0;           /* the library writes nothing while the count is 0 */
        const mwSize d3[3] = {on * (mwSize)t->n, on * (mwSize)t->P, on * (mwSize)t->g};
        mxArray *o[4];                               /* the sizes the library writes */
        o[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        o[1] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        o[2] = mxCreateDoubleMatrix(on * (mwSize)t->P, on * (mwSize)t->g, mxREAL);
        o[3] = mxCreateDoubleScalar((double)cnt);
        if (cnt > 0) ck(t->h, dcfm_get_imputed(t->h, mxGetDoubles(o[0]), mxGetDoubles(o[1]), mxGetDoubles(o[2]), &cnt));
        for (int i = 0; i < 4; ++i)
            if (i == 0 || i < nlhs) plhs[i] = o[i];
            else mxDestroyArray(o[i]);
    } else if (!strcmp(cmd, "set_regression")) {     /* dcfm_mex('set_regression', h, resp) */
        nargs(nrhs, 3, cmd);
        /* the argument that needs no handle first: a malformed call never reaches the library */
        const mxArray *r = prhs[2];
        if (!mxIsDouble(r) || mxIsComplex(r) || mxGetNumberOfElements(r) > 32)
            mexErrMsgIdAndTxt("dcfm:arg", "resp must be a real double vector of at most 32 1-based indices, or empty");
        const int32_t q = (int32_t)mxGetNumberOfElements(r);
        int64_t resp[32];
        for (int32_t j = 0; j < q; ++j) {
            const double v = mxGetDoubles(r)[j];
            if (!(v >= 1.0 && v <= 2147483647.0) || v != (double)(int64_t)v)
                mexErrMsgIdAndTxt("dcfm:arg", "resp must hold positive integers (1-based indices)");
            resp[j] = (int64_t)v - 1;
        }
        slot *t = get(prhs[1]);
        for (int32_t j = 0; j < q; ++j)
            if (resp[j] >= t->P * t->g)
                mexErrMsgIdAndTxt("dcfm:arg", "resp must lie in 1 .. p = %lld", (long long)(t->P * t->g));
        ck(t->h, dcfm_set_regression(t->h, q > 0 ? resp : NULL, q));
        t->rq = q;
    } else if (!strcmp(cmd, "regression")) {         /* [coef, coef_m2, rcov, rcov_m2, r2, r2_m2, count] = ... */
        nargs(nrhs, 2, cmd);
        slot *t = get(prhs[1]);
        int64_t cnt = 0;
        ck(t->h, dcfm_get_regression(t->h, NULL, NULL, NULL, NULL, NULL, NULL, &cnt));
        const mwSize on = cnt > 0 ? 1 : 0;           /* the library writes nothing while the count is 0 */
        const mwSize p = on * (mwSize)(t->P * t->g), q = on * (mwSize)t->rq;
        mxArray *o[7];                               /* the sizes the library writes */
        o[0] = mxCreateDoubleMatrix(p, q, mxREAL);
        o[1] = mxCreateDoubleMatrix(p, q, mxREAL);
        o[2] = mxCreateDoubleMatrix(q, q, mxREAL);
        o[3] = mxCreateDoubleMatrix(q, q, mxREAL);
        o[4] = mxCreateDoubleMatrix(q, on, mxREAL);
        o[5] = mxCreateDoubleMatrix(q, on, mxREAL);
        o[6] = mxCreateDoubleScalar((double)cnt);
        if (cnt > 0)
            ck(t->h, dcfm_get_regression(t->h, mxGetDoubles(o[0]), mxGetDoubles(o[1]), mxGetDoubles(o[2]),
                                         mxGetDoubles(o[3]), mxGetDoubles(o[4]), mxGetDoubles(o[5]), &cnt));
        for (int i = 0; i < 7; ++i)
            if (i == 0 || i < nlhs) plhs[i] = o[i];
            else mxDestroyArray(o[i]);
    } else if (!strcmp(cmd, "destroy")) {
        nargs(nrhs, 2, cmd);
        slot *t = get(prhs[1]);
        dcfm_destroy(t->h);
        t->h = 0;
        mexUnlock();
    } else {
        mexErrMsgIdAndTxt("dcfm:cmd", "unknown command %s", cmd);
    }
}
