/*
 * dcfm.h — C ABI of the MI355X-native Gibbs sweep + covariance assembly for the
 * divide-and-conquer sparse latent-factor model (Sabnis & Pati, arXiv 1612.02875).
 *
 * Drop-in boundary.  The reference has no plugin or operator
 * API: its only interface is the MATLAB function
 *     Sigmaout = divideconquer(Y,g,k,BURNIN,MCMC,thin,rho)      (divideconquer.m:1)
 * and the boundary sits INSIDE it, between the driver (dc:29-87: zero-column
 * removal, partition, standardisation, hyper-parameters, initial draws) and the
 * iteration loop (dc:90-197).  These entry points take over exactly the loop's
 * read/write set; a MEX gateway or the Python host twin
 * (package ``dcfm_amd``, ctypes) calls them.
 *
 * Conventions
 *  - Plain C, no exceptions cross the ABI.  Every int-returning call returns
 *    DCFM_OK (0) or a DCFM_ERR_* code; dcfm_last_error() gives the message.
 *  - Host arrays are MATLAB column-major with the reference's shapes (so a MEX
 *    gateway passes mxGetPr/mxGetDoubles pointers straight through).  The
 *    caller owns every host buffer; the library copies and never keeps a
 *    caller pointer.
 *  - "local" arrays cover the shards this rank owns: global shards
 *    [shard0, shard0 + g_local) with g_local = g / nranks, shard0 = rank*g_local.
 *  - A handle is not thread-safe.  One process (one host thread) per GPU.
 *  - dcfm_run is asynchronous w.r.t. the host (work is queued on the handle's
 *    HIP stream); dcfm_get_*, dcfm_synchronize block.
 */
#ifndef DCFM_H
#define DCFM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCFM_ABI_VERSION 2

/* status codes */
#define DCFM_OK              0
#define DCFM_ERR_INVALID     1   /* bad argument / shape / call order            */
#define DCFM_ERR_UNSUPPORTED 2   /* valid for the reference, not yet built here  */
#define DCFM_ERR_HIP         3   /* HIP runtime error (incl. no device)          */
#define DCFM_ERR_RCCL        4   /* RCCL error                                   */
#define DCFM_ERR_NUMERIC     5   /* non-finite state detected                    */
#define DCFM_ERR_ALLOC       6   /* device or host allocation failed             */

/* dcfm_config.flags */
#define DCFM_FLAG_INJECT_DRAWS 0x1u  /* read standard variates from dcfm_set_draws
                                        buffers instead of on-device Philox        */
#define DCFM_FLAG_UNFUSED      0x2u  /* K <= 32 through the per-kernel side-stream layout
                                        (k_prep / k_xchol on a second stream, k_draws
                                        batches) instead of the fused launch chain;
                                        same results (tests, diagnostics)           */
#define DCFM_FLAG_ONE_STREAM   0x4u  /* every launch on one stream (isolated timings) */
#define DCFM_FLAG_FLAT_PRIORITY 0x8u /* default priority for every stream          */
#define DCFM_FLAG_COMM_SELF    0x20u  /* one rank through the collective data path with a
                                        real one-rank RCCL communicator (dcfm_comm_init):
                                        exercises the RCCL calls on a one-GPU box; same
                                        results as the plain one-rank chain (tests)        */
#define DCFM_FLAG_EXACT_RESIDUAL 0x10u /* ps / omega (dc:169-171) from the direct residual
                                        sum((Yd - eta*Lambda').^2), one extra pass over Y
                                        (k_resid), instead of the SS identity inside the
                                        loading-row kernel (parity runs)   */
#define DCFM_FLAG_GUARD_ALL    0x40u  /* the SS-identity guard rejects every row: the default
                                        path's own residual fallback (K <= 32: resid_rows8 in
                                        the loading-row kernel; K > 32: every tile through
                                        k_resid_flagged) for every row (tests)            */
#define DCFM_FLAG_SIGMA_M2     0x80u  /* also accumulate the element-wise second moment of the
                                        per-sample Sigma (a second buffer the size of this rank's
                                        Sigmaout block, one more assembly kernel per flush), for
                                        dcfm_get_sigma_moment's M2 and SD; off: nothing is
                                        allocated or launched                              */
#define DCFM_FLAG_PRECISION_MEAN 0x100u /* also accumulate the posterior mean of the precision matrix,
                                        (1/effsamp) sum_s Sigma(s)^-1 (one more buffer the size of this
                                        rank's Sigmaout block, the per-sample omega slots, a factor
                                        buffer and the kernels of precision_mean.hip per flush), for
                                        dcfm_get_precision_mean[_cols]; off: nothing is allocated or
                                        launched                                          */
#define DCFM_FLAG_PARTIAL_CORR 0x200u  /* also accumulate the posterior mean and second moment of the
                                        per-sample partial correlations (two more buffers the size of
                                        this rank's Sigmaout block; the per-sample omega slots, factor
                                        buffer and panel kernels it shares with PRECISION_MEAN, plus the
                                        kernels of partial_corr.hip per flush), for
                                        dcfm_get_partial_corr[_cols]; off: nothing is allocated or
                                        launched                                          */
#define DCFM_FLAG_CORR         0x400u  /* also accumulate the posterior mean and second moment of the
                                        per-sample correlation matrix D(s)^-1/2 Sigma(s) D(s)^-1/2 and of
                                        the communalities (two more buffers the size of this rank's
                                        Sigmaout block, the per-sample omega slots, a p x asm_batch scale
                                        array, two p-vectors and the two kernels of corr.hip per flush),
                                        for dcfm_get_corr[_cols] and dcfm_get_communality; off: nothing
                                        is allocated or launched                           */
#define DCFM_FLAG_REGRESSION   0x800u  /* allow dcfm_set_regression: the per-sample omega slots, the factor
                                        buffer and the panel scratch that DCFM_FLAG_PARTIAL_CORR alone
                                        allocates (no p x p accumulator: dcfm_sigma_block's bytes do not
                                        change); the panel kernels and the two kernels of regression.hip
                                        run per flush once a response set is given; off: nothing is
                                        allocated or launched                              */

typedef struct dcfm_handle dcfm_handle;

/* Replaces the scalars the loop reads: dc:41 (P, K), dc:45 (N, effsamp),
 * dc:62-65 (hyper-parameters), plus build-side placement and RNG settings. */
typedef struct {
    int32_t n;          /* observations (rows of Y), dc:30                       */
    int32_t P;          /* variables per shard, P = p/g, dc:41.  P = 1 is
                         * supported with the reference's semantics: dc:156's
                         * mat is then 1 x K and MATLAB's sum runs along it, so
                         * dc:157 / dc:161 use (sum tau_l)(sum s_l) over l >= h
                         * (csrc/delta.h, quirk Q14)                              */
    int32_t g;          /* total number of shards (groups), dc:1                 */
    int32_t K;          /* factors per shard, K = k/g, dc:41                     */
    double  rho;        /* correlation of the shared factor, dc:1                */
    int64_t burnin;     /* BURNIN, dc:1                                          */
    int64_t mcmc;       /* MCMC, dc:1;  effsamp = mcmc/thin (dc:45, quirk Q8)    */
    int64_t thin;       /* thin, dc:1                                            */
    double  as_, bs, df, ad1, bd1, ad2, bd2;  /* dc:62-65 (1,0.3,3,2,1,2,1)      */
    uint64_t seed;      /* Philox key (counter-based RNG; ignored with INJECT)   */
    int32_t nranks;     /* ranks sharing the chain (1 = single GPU)              */
    int32_t rank;       /* this rank                                             */
    int32_t device;     /* HIP device ordinal this handle runs on                */
    uint32_t flags;     /* DCFM_FLAG_*                                           */
    int32_t asm_batch;  /* saved samples per covariance-assembly flush (0 = 32)  */
    int32_t reserved[7];
} dcfm_config;

/* Sampler state (dc:69-87, updated by dc:90-177).  All column-major.
 * NULL members are skipped by get, and are an error for set unless noted. */
typedef struct {
    double *Lambda;  /* P x K x g_local   loadings                  (dc:70,144) */
    double *ps;      /* P x 1 x g_local   residual precisions       (dc:69,170) */
    double *omega;   /* P x g_local       diag(Omega) (Q1: = ps at init,
                                          = 1./ps after dc:171)                 */
    double *psi;     /* P x K x g_local   psijh                     (dc:73,150) */
    double *Plam;    /* P x K x g_local   loading precisions        (dc:77,176) */
    double *X;       /* n x K             shared factor, replicated (dc:71,128) */
    double *Z;       /* n x K x g_local   shard factors             (dc:71,106) */
    double *eta;     /* n x K x g_local   get only; set ignores it (Q12)        */
    double *delta;   /* K x 1 x g         ALL shards (replicated)   (dc:74,163) */
    double *tauh;    /* K x 1 x g         ALL shards (replicated)   (dc:76,163) */
} dcfm_state_view;

/* Injected standard variates, ALL shards, column-major,
 * one trailing iteration dimension of length n_iter:
 *   NZ K x n x g x T (dc:104)   NX K x n x T (dc:126)   NL K x P x g x T (dc:142)
 *   Gpsi P x K x g x T  standard gamma, shape df/2+0.5       (dc:150)
 *   Gdelta K x g x T    shape ad1+P*K/2 (h=1), ad2+P*(K-h+1)/2 (dc:158,163)
 *   Gps P x g x T       shape as+n/2                           (dc:170)     */
typedef struct {
    const double *NZ, *NX, *NL, *Gpsi, *Gdelta, *Gps;
} dcfm_draws_view;

/* ---- lifecycle ---------------------------------------------------------- */
int  dcfm_create(const dcfm_config *cfg, dcfm_handle **out);
void dcfm_destroy(dcfm_handle *h);
const char *dcfm_last_error(const dcfm_handle *h);   /* h may be NULL */
int  dcfm_abi_version(void);

/* ---- multi-rank: RCCL communicator over xGMI ----------------------------
 * Rank 0 calls dcfm_comm_unique_id, the host broadcasts the 128 bytes
 * (torch.distributed / MPI / files — any side channel), every rank calls
 * dcfm_comm_init.  Not needed when nranks == 1. */
int  dcfm_comm_unique_id(uint8_t out[128]);
int  dcfm_comm_init(dcfm_handle *h, const uint8_t id[128]);
/* Test communicator: the n handles (nranks = n, ranks 0..n-1, one device) exchange
 * through device copies inside this process instead of RCCL, each handle driven by
 * its own host thread — the multi-rank sweep on a single GPU.  Same collective
 * semantics and call order as dcfm_comm_init. */
int  dcfm_comm_init_loopback(dcfm_handle *const *handles, int32_t n);

/* ---- inputs -------------------------------------------------------------- */
/* Yd(:,:,shard0+1 : shard0+g_local) after dc:48-59, n x P x g_local.        */
int  dcfm_set_data(dcfm_handle *h, const double *Yd_local);
/* On-device ingest (replaces the host's dc:48-59): Y is the raw
 * n x p_in matrix (column-major, after the caller's zero-column removal, dc:31-39, or
 * before it — cols index Y's own columns); cols[m*P + j] (0-based) is the input column
 * of local shard m, position j, i.e. keep(varind((shard0+m)*P + j)) - 1 in MATLAB terms.
 * Y goes to HBM once; the kernel gathers, centres, scales by 1./sqrt(var) (n - 1) and
 * lays Yd out for the sweep.  sd_out (nullable): P x g_local sample standard deviations
 * (for unpermute_sigma); dev_ms (nullable): the kernel's device time.  A constant
 * column (zero variance, Q13) is DCFM_ERR_INVALID; needs n >= 2. */
int  dcfm_set_data_raw(dcfm_handle *h, const double *Y, int64_t p_in, const int64_t *cols,
                       double *sd_out, double *dev_ms);
/* Yd as the sweep holds it, n x P x g_local column-major (the layout of dcfm_set_data). */
int  dcfm_get_data(dcfm_handle *h, double *Yd_local);
/* dc:31-34 on the device: nnz_out[j] = nnz(Y(:,j)) for the n x p column-major Y (NaN
 * counts as non-zero).  No handle: the kept width p (hence P = p/g) is not known yet. */
int  dcfm_count_nonzero_columns(int device, const double *Y, int32_t n, int64_t p, int32_t *nnz_out,
                                double *dev_ms);
int  dcfm_set_state(dcfm_handle *h, const dcfm_state_view *s);
/* Initial state on the device (dc:68-87), instead of dcfm_set_state:
 * ps = Ga(as)/bs, omega = ps (Q1), X, Z ~ N(0,1), psijh = (2/df) Ga(df/2), delta(1) =
 * bd1 Ga(ad1), delta(2:K) = bd2 Ga(ad2), tauh = cumprod, Plam = psijh .* tauh', Lambda = 0,
 * from the handle's Philox key at iteration-0 counters (sites 7-12; variate e of a shard
 * = MATLAB linear index e inside that shard's array, counter row e/32, index e%32 — as
 * dcfm_rng_fill, which reproduces them).  Identical on any number of ranks. */
int  dcfm_init_state(dcfm_handle *h);
/* Draws for iterations first_iter .. first_iter+n_iter-1 (1-based, as iter). */
int  dcfm_set_draws(dcfm_handle *h, const dcfm_draws_view *d, int64_t first_iter, int64_t n_iter);

/* ---- the hot loop (dc:90-197) ------------------------------------------- */
/* Runs iterations first_iter .. first_iter+n_iter-1 (1-based).  Saved
 * iterations (mod(iter,thin)==0 && iter>burnin, dc:180) feed the covariance
 * assembly (dc:182-195); pending saved samples are flushed before return.   */
int  dcfm_run(dcfm_handle *h, int64_t first_iter, int64_t n_iter);
int  dcfm_synchronize(dcfm_handle *h);

/* ---- outputs ------------------------------------------------------------ */
int  dcfm_get_state(dcfm_handle *h, dcfm_state_view *out);
/* dcfm_get_state without the non-finite check: after a dcfm_run that ended in
 * DCFM_ERR_NUMERIC, the state as the device holds it (NaN / Inf included), so a
 * caller can see which stage of the failing iteration went non-finite.  The
 * handle stays in its error state until set_state / init_state. */
int  dcfm_get_state_raw(dcfm_handle *h, dcfm_state_view *out);
/* Sigmaout, p x p (p = P*g), symmetric, in the reference's permuted and
 * standardised coordinates (dc:186-195, quirk Q7).  Collective when
 * nranks > 1: every rank must call it; rank 0 receives the matrix (out may be
 * NULL on the other ranks and is not written there).  Sigmaout is block-sharded
 * over the ranks (dcfm_sigma_block): the read-out moves each element once, from
 * its owner to rank 0 (RCCL send/recv), in column stripes of <= 2 GiB. */
int  dcfm_get_sigma(dcfm_handle *h, double *out);
/* Columns col0 .. col0+ncols-1 of Sigmaout: p x ncols column-major, i.e. exactly
 * out = Sigmaout(:, col0+1 : col0+ncols) — a contiguous chunk of the MATLAB array,
 * so a caller can fill a p x p result stripe by stripe (config c5: 80 GB) with
 * device scratch of only p x ncols.  Collective when nranks > 1; the stripe goes
 * to rank 0 only (as dcfm_get_sigma). */
int  dcfm_get_sigma_cols(dcfm_handle *h, int64_t col0, int64_t ncols, double *out);
/* This rank's block of Sigmaout (the build's output sharding; the reference holds
 * the whole p x p, dc:42): out[0], out[1] = the rows [row0, row1) whose lower
 * triangle it accumulates (contiguous 128-row tiles, balanced by tile count over
 * the ranks), out[2] = its device bytes for Sigmaout (~p^2 / (2 nranks) * 8; once more
 * with DCFM_FLAG_SIGMA_M2, the second moment beside the mean, and once more with
 * DCFM_FLAG_PRECISION_MEAN, the precision accumulator, and twice more with
 * DCFM_FLAG_PARTIAL_CORR, the two moments of the partial correlations, and twice more with
 * DCFM_FLAG_CORR, the two moments of the correlations). */
int  dcfm_sigma_block(const dcfm_handle *h, int64_t out[3]);
int64_t dcfm_saved_samples(const dcfm_handle *h);
/* Posterior moments of Sigma's entries.  With Sigma(s) the matrix dc:182-192 builds from saved
 * sample s (Sigma(s)_ab = c_ab Lambda(s)_a . Lambda(s)_b + [a == b] omega(s)_a, c_ab = 1 inside a
 * shard, rho across), `which` selects
 *   DCFM_SIGMA_MEAN  Sigmaout = (1/effsamp) sum_s Sigma(s): exactly dcfm_get_sigma_cols;
 *   DCFM_SIGMA_M2    M2 = (1/effsamp) sum_s Sigma(s).^2, the same effsamp = mcmc/thin scaling
 *                    (quirk Q8) as the mean;
 *   DCFM_SIGMA_SD    sqrt(max(0, r M2 - (r Sigmaout).^2)), r = effsamp / dcfm_saved_samples(h):
 *                    the posterior standard deviation (population form, 1/S) over the samples
 *                    saved so far, whatever effsamp is; formed on the device from both buffers.
 * M2 and SD need DCFM_FLAG_SIGMA_M2 (else DCFM_ERR_INVALID); SD with no saved sample is
 * DCFM_ERR_INVALID.  M2 - mean^2 cancels: an entry keeps about eps M2 / var relative accuracy.
 * Layout, striping and collective semantics as dcfm_get_sigma_cols / dcfm_get_sigma. */
#define DCFM_SIGMA_MEAN 0
#define DCFM_SIGMA_M2   1
#define DCFM_SIGMA_SD   2
int  dcfm_get_sigma_moment_cols(dcfm_handle *h, int32_t which, int64_t col0, int64_t ncols, double *out);
int  dcfm_get_sigma_moment(dcfm_handle *h, int32_t which, double *out);
/* Posterior mean of the precision matrix (DCFM_FLAG_PRECISION_MEAN at dcfm_create, else
 * DCFM_ERR_INVALID): Theta = (1/effsamp) sum_s Sigma(s)^-1 over the saved samples, Sigma(s) the
 * per-sample matrix of dc:182-192, with the same effsamp = mcmc/thin scaling (quirk Q8) as Sigmaout;
 * all zeros before the first saved sample.  This is E[Sigma^-1 | Y], not the inverse of the posterior
 * mean (dcfm_sigma_solve).  Accumulated on the device tile by tile from thin factor panels (Sigma(s)^-1
 * is block-diagonal plus low rank, as Sigma(s) is): no p x p factorisation.  An entry is accurate to
 * first order in eps cond(Sigma(s)).  p x p in Sigmaout's coordinates, symmetric bit for bit; layout,
 * striping and collective semantics as dcfm_get_sigma_cols / dcfm_get_sigma. */
int  dcfm_get_precision_mean_cols(dcfm_handle *h, int64_t col0, int64_t ncols, double *out);
int  dcfm_get_precision_mean(dcfm_handle *h, double *out);
/* Posterior moments of the partial correlations (DCFM_FLAG_PARTIAL_CORR at dcfm_create, else
 * DCFM_ERR_INVALID).  With Theta(s) = Sigma(s)^-1 of saved sample s (Sigma(s) the per-sample matrix of
 * dc:182-192) and d_a(s) = Theta(s)_aa, the per-sample partial-correlation matrix is
 *   R(s)_ab = -Theta(s)_ab / sqrt(d_a(s) d_b(s))  (a != b),   R(s)_aa = 1 exactly,
 * and `which` selects
 *   DCFM_SIGMA_MEAN  PC  = (1/effsamp) sum_s R(s), with the same effsamp = mcmc/thin scaling (quirk Q8)
 *                    as Sigmaout: its diagonal is exactly 1 * saved / effsamp (the count of the saved
 *                    samples scaled, not a computed product);
 *   DCFM_SIGMA_M2    PC2 = (1/effsamp) sum_s R(s).^2, the same scaling;
 *   DCFM_SIGMA_SD    sqrt(max(0, r PC2 - (r PC).^2)), r = effsamp / dcfm_saved_samples(h): the posterior
 *                    standard deviation (population form) over the samples saved so far; 0 on the diagonal.
 * R(s) is not linear in Sigma(s)^-1: PC is the posterior mean of the partial correlation, not the plug-in
 * -T_ab / sqrt(T_aa T_bb) of the precision mean T, and the SD is what tells an edge of the graphical model
 * from noise.  All zeros before the first saved sample; SD with no saved sample and a `which` outside the
 * three are DCFM_ERR_INVALID.  Accumulated on the device tile by tile from the thin factor panels of
 * Sigma(s)^-1, each row scaled by 1 / sqrt(d_a(s)) (a non-positive d_a(s) gives NaN, which runs through):
 * an entry of R(s) is accurate to first order in eps cond(Sigma(s)), and |R(s)_ab| <= 1.  M2 - mean^2
 * cancels: an entry's variance keeps about eps PC2 / var relative accuracy.  Device bytes: twice this
 * rank's Sigmaout block (dcfm_sigma_block), plus -- shared with DCFM_FLAG_PRECISION_MEAN, whose accumulator
 * is not allocated for this flag alone -- the factor buffer p x 4 round_up(asm_batch K, 16) doubles, the
 * (2 g + 1) asm_batch K^2 scratch and the omega slots 2 p asm_batch.  p x p in Sigmaout's coordinates,
 * symmetric bit for bit; layout, striping and collective semantics as dcfm_get_sigma_moment[_cols]. */
int  dcfm_get_partial_corr_cols(dcfm_handle *h, int32_t which, int64_t col0, int64_t ncols, double *out);
int  dcfm_get_partial_corr(dcfm_handle *h, int32_t which, double *out);
/* Posterior moments of the (marginal) correlation matrix and of the communalities (DCFM_FLAG_CORR at
 * dcfm_create, else DCFM_ERR_INVALID).  The columns are standardised before the sweep (dc:57-59), but the
 * diagonal of Sigma(s) is not 1: v_a(s) = Sigma(s)_aa = |Lambda_a(s)|^2 + omega_a(s) moves from sample to
 * sample.  Per saved sample s, with c_ab = 1 for a, b in one shard and rho across (dc:186-189),
 *   R(s)_ab = c_ab Lambda_a(s) . Lambda_b(s) / sqrt(v_a(s) v_b(s))  (a != b),   R(s)_aa = 1 exactly,
 *   h_a(s)  = |Lambda_a(s)|^2 / v_a(s)          the communality: the share of variable a's variance that the
 *                                               factors explain (invariant to a rotation of the factors),
 * and `which` selects, for dcfm_get_corr[_cols] (p x p) and dcfm_get_communality (p doubles) alike,
 *   DCFM_SIGMA_MEAN  (1/effsamp) sum_s R(s) resp. h(s), with the same effsamp = mcmc/thin scaling (quirk Q8)
 *                    as Sigmaout: the diagonal of the matrix is exactly saved / effsamp;
 *   DCFM_SIGMA_M2    (1/effsamp) sum_s R(s).^2 resp. h(s).^2, the same scaling;
 *   DCFM_SIGMA_SD    sqrt(max(0, r M2 - (r MEAN).^2)), r = effsamp / dcfm_saved_samples(h): the posterior
 *                    standard deviation (population form) over the samples saved so far; 0 on the diagonal.
 * The mean is the posterior mean of the per-sample correlation, not the plug-in D^-1/2 Sigmaout D^-1/2, and it
 * comes with an SD.  All zeros before the first saved sample; SD with no saved sample and a `which` outside
 * the three are DCFM_ERR_INVALID.  No inversion is involved and |R(s)_ab| <= 1: an entry of R(s) is accurate
 * to about (2 K + 8) eps whatever the conditioning of Sigma(s); a non-finite or non-positive v_a(s) gives NaN,
 * which runs through.  M2 - mean^2 cancels: an entry's variance keeps about eps M2 / var relative accuracy.
 * Device bytes: twice this rank's Sigmaout block (dcfm_sigma_block), plus p (asm_batch + 2) doubles and the
 * omega slots 2 p asm_batch.  The matrix is in Sigmaout's coordinates, symmetric bit for bit; layout, striping
 * and collective semantics as dcfm_get_sigma_moment[_cols].  dcfm_get_communality is not collective: every
 * rank holds all p entries (bitwise equal on all ranks) and `out` must not be NULL on any rank. */
int  dcfm_get_corr_cols(dcfm_handle *h, int32_t which, int64_t col0, int64_t ncols, double *out);
int  dcfm_get_corr(dcfm_handle *h, int32_t which, double *out);
int  dcfm_get_communality(dcfm_handle *h, int32_t which, double *out);
/* Error of Sigmaout against a truth Sigma0 = U U' + diag(s) given in the same permuted,
 * standardised coordinates (U: p x r column-major, r <= 32; s: p), computed on the
 * device (Sigmaout never leaves HBM; c5: 80 GB).  out[0] = ||Sigmaout - Sigma0||_F,
 * out[1] = ||Sigma0||_F, out[2] = ||Sigmaout - Sigma0||_2 from `iters` Lanczos steps
 * (seeded start, full reorthogonalisation; exact when iters >= p; 0 skips it).  The
 * reference leaves this to the caller (Frobenius and
 * operator-norm error against the synthetic truth).  Collective when nranks > 1. */
int  dcfm_sigma_error(dcfm_handle *h, const double *U, int32_t r, const double *s, int32_t iters,
                      uint64_t seed, double out[3]);

/* ---- Sigmaout as a linear operator -----------------------------------------
 * Sigmaout is too big to move (1.6 GB of stored triangle at c3, 80 GB over the ranks at c5), so
 * the products a covariance is estimated for -- projections, quadratic forms, principal
 * components -- are taken where it lies.
 *
 * dcfm_sigma_apply: out = Sigmaout * V.  V and out are p x nv column-major host arrays (p = P*g,
 * nv >= 1, in Sigmaout's permuted, standardised coordinates); the result equals
 * dcfm_get_sigma(h) times V (the mean accumulator, with the read-out's effsamp scaling), up to the
 * rounding of a length-p dot product in another summation order.  One kernel pass serves up to 32
 * columns and reads every stored 128 x 128 tile of the lower triangle once (fp64 MFMA, both the
 * tile and its mirror from the one read), so a pass moves about 4 p^2 bytes whatever nv <= 32 is;
 * a larger nv runs in chunks of 32 inside the call.  No atomics: the same inputs give the same bits
 * on every call.  dev_ms (nullable): the accumulated device time of the kernel passes.
 * Collective when nranks > 1: every rank calls it with the same V, multiplies the tiles it owns,
 * and receives the full product (an all-reduce of p x nv).  Works with and without
 * DCFM_FLAG_SIGMA_M2 and never reads the second moment.  Device scratch (the V and out blocks and
 * the tiles' partial panels, about p^2 nv' / 128 doubles with nv' = 16 or 32) is allocated inside
 * the call and freed before it returns.
 * Errors: NULL handle ("null handle") or NULL V / out ("null argument"), nv < 1: DCFM_ERR_INVALID. */
int  dcfm_sigma_apply(dcfm_handle *h, const double *V, int32_t nv, double *out, double *dev_ms);
/* dcfm_sigma_eigs: the r largest eigenpairs of Sigmaout, 1 <= r <= min(32, p), by a block Krylov
 * (block Lanczos) iteration with Rayleigh-Ritz: a seeded normal start block of width b = min(32, p),
 * one dcfm_sigma_apply pass per step, the new block re-orthogonalised twice against the whole basis
 * and within itself (columns falling below 1e-13 of their norm are dropped, so a rank-deficient block
 * puts no NaN into the basis).  It stops when max_i resid_i <= tol * lambda_1, after max_passes
 * passes, or when the basis spans all p dimensions (then the result is exact); reaching max_passes
 * unconverged is NOT an error -- the call returns DCFM_OK and the caller reads resid.
 *   evals[r]    descending
 *   evecs       nullable; p x r column-major, orthonormal columns, the entry of largest magnitude of
 *               each column positive (lowest index on ties): comparable across runs and ranks
 *   resid[r]    ||Sigmaout v_i - lambda_i v_i||_2 from a real dcfm_sigma_apply pass on the returned
 *               vectors (not the Ritz estimate)
 *   passes      nullable; block applies of the iteration (the residual pass on the r vectors, and
 *               a pass that checked a not-yet-converged candidate, are not counted)
 * The basis (p x passes*b doubles, twice) and the projected eigenproblem (at most max_passes*b wide,
 * solved by csrc/symeig.h: no LAPACK) stay on the host, as dcfm_sigma_error's Lanczos basis does;
 * Sigmaout never leaves HBM.  Collective when nranks > 1: every rank runs the same host arithmetic
 * on the same all-reduced bytes and returns identical results.
 * Errors (DCFM_ERR_INVALID): NULL handle, NULL evals / resid, r outside 1..min(32, p), tol <= 0,
 * max_passes < 1, no saved sample yet (dcfm_saved_samples == 0). */
int  dcfm_sigma_eigs(dcfm_handle *h, int32_t r, double tol, int32_t max_passes, uint64_t seed,
                     double *evals, double *evecs, double *resid, int32_t *passes);
/* dcfm_sigma_solve: X = Sigmaout^{-1} B by conjugate gradients on dcfm_sigma_apply's pass, with the
 * whole iteration on the device.  B and X are p x nv column-major host arrays (nv >= 1, Sigmaout's
 * permuted, standardised coordinates); Sigmaout X = B for the operator dcfm_sigma_apply multiplies
 * by, which is symmetric positive definite once a sample is saved (a mean of Lambda C Lambda' +
 * diag(omega), omega > 0) with a diagonal of about 1, so the iteration is plain CG, no preconditioner.
 * The columns are solved independently and in lock-step: each has its own alpha, beta and stop test,
 * and one pass serves up to 32 of them (this is not O'Leary's block CG: no nv x nv solves, no
 * rank-deficiency breakdown); a larger nv runs in chunks of 32 inside the call.  Between the upload
 * of a chunk of B and the download of its X no p-length vector crosses the bus: per step the host
 * reads the columns' done flags.
 * A column stops when its recurrence residual satisfies ||r_c|| <= tol ||B_c||, or after max_iter
 * steps; reaching max_iter is NOT an error -- the call returns DCFM_OK and the caller reads relres.
 * A stopped column is frozen (its X, r, p untouched by later steps).  A column with B_c = 0 returns
 * X_c = 0 exactly with iters 0, and a column whose p' Sigmaout p is <= 0 or not finite is frozen at
 * its current iterate, so no NaN from a division reaches X.
 *   relres[nv]  ||B_c - Sigmaout X_c||_2 / ||B_c||_2 from a real pass on the returned X (not the
 *               recurrence's estimate); 0 where B_c = 0
 *   iters[nv]   nullable; CG steps taken by each column
 *   quad[nv]    nullable; B_c' X_c, formed on the device: the quadratic form b' Sigmaout^{-1} b
 *   dev_ms      nullable; accumulated device time of the call's kernels (passes and panel kernels)
 * No atomics: the same inputs give the same bits, and a column's bits do not depend on which other
 * columns share its call.  Collective when nranks > 1: every rank calls with the same B, keeps the
 * panels replicated and runs the same vector kernels on the same all-reduced bytes of the pass, so
 * the stop decisions (and the number of collective calls) are identical and every rank receives
 * identical X.  Works with and without DCFM_FLAG_SIGMA_M2.  Device scratch (dcfm_sigma_apply's plus
 * three p x min(nv, 32) panels) is allocated inside the call and freed before it returns.
 * Errors (DCFM_ERR_INVALID): NULL handle ("null handle"), NULL B / X / relres ("null argument"),
 * nv < 1, tol <= 0 or not finite, max_iter < 1, no saved sample yet (dcfm_saved_samples == 0). */
int  dcfm_sigma_solve(dcfm_handle *h, const double *B, int32_t nv, double tol, int32_t max_iter,
                      double *X, double *relres, int32_t *iters, double *quad, double *dev_ms);

/* ---- chain trace (convergence diagnostics across chains) ----
 * dcfm_set_trace(h, cap): record one row per iteration of later dcfm_run calls, up to cap
 * rows (0 = off, the default; resets the count).  Row = this rank's local-shard sums
 *   [ ||Lambda||_F^2,  sum omega (= tr Omega),  sum log ps,  sum_m sum_h log tau_h^m ]
 * after the iteration (tr of the iteration's Sigma draw = row[0] + row[1], dc:185); ranks
 * that split one chain add their rows.  dcfm_get_trace: out (nullable) gets count x 4
 * doubles, row-major. */
int  dcfm_set_trace(dcfm_handle *h, int64_t capacity);
int  dcfm_get_trace(dcfm_handle *h, double *out, int64_t *count);

/* ---- per-sample draws of V' Sigma V (posterior uncertainty of any functional) ----
 * The read-outs above describe the posterior mean of Sigma, and DCFM_FLAG_SIGMA_M2 one standard
 * deviation per entry.  A quantity that is not a single entry -- the variance v' Sigma v of a portfolio
 * or contrast, a correlation Sigma_ab / sqrt(Sigma_aa Sigma_bb), a ratio of variances, a credible
 * interval for any of them -- needs its value per saved sample.  With Sigma(s) the matrix dc:182-192
 * builds from saved sample s, the library records Q(:,:,s) = V' * Sigma(s) * V for a caller-chosen block
 * V, from one read of Lambda and V per saved sample (Sigma(s) is never formed): with W_m = Lambda_m' V_m,
 * W = sum_m W_m,  V' Sigma(s) V = rho W'W + sum_m [(1 - rho) W_m'W_m + V_m' diag(omega_m) V_m].
 *
 * dcfm_set_probes: V is a p x nv column-major host array (p = P*g, 1 <= nv <= 32) in Sigmaout's permuted,
 * standardised coordinates, as for dcfm_sigma_apply; every rank passes the same full V and keeps the rows
 * of its own shards on the device.  From the next dcfm_run on, every saved sample (mod(iter,thin)==0 &&
 * iter>burnin, dc:180) records one draw until `capacity` draws are held; later saved samples are not
 * recorded (as dcfm_set_trace).  Calling it again replaces V and resets the count.  capacity == 0 (V may
 * then be NULL, nv is ignored) turns the feature off and frees its buffers; until a call with
 * capacity > 0 nothing is allocated and nothing is launched.  Needs neither data nor state nor a
 * communicator and is not collective.  The kernel runs behind k_save on the sweep stream and its device
 * time is booked under DCFM_K_SAVE.  No floating-point atomics and fixed summation orders: the same
 * inputs give the same bits on every run.
 * Device bytes: 8 (P g_local nv + capacity * slot + scratch), with slot = nv^2 on one rank (the draw
 * itself) and K nv + nv^2 on several (the rank's partial W and its partial of the bracket above), and
 * scratch = (g_local (s + 1) + ceil(g_local / 8)) (K nv + nv^2) doubles of slice, shard and shard-group
 * partials (s = min(32, max(1, 256 / g_local)) slices per shard) plus a ticket word for each.
 * Errors (DCFM_ERR_INVALID, a block set before stays as it was): NULL handle ("null handle"), NULL V with
 * capacity > 0 ("null argument"), nv outside 1..32, capacity < 0, a non-finite entry in V.
 *
 * dcfm_get_probe_draws: count (required) receives the number of draws held; out (nullable) the nv x nv x
 * count column-major array Q above, in saved-sample order.  Sigma(s) is the per-sample matrix itself,
 * without the effsamp scaling: sum(Q,3) / effsamp equals V' * Sigmaout * V up to rounding.  Every slice
 * is symmetric bit for bit (one triangle computed, then mirrored).  Blocks (synchronises the sweep
 * stream) and does not disturb a later dcfm_run.  With nranks > 1 it is collective: every rank calls it,
 * the ranks' partials of all draws travel in one all-gather (nothing p-length crosses the bus), are
 * summed in rank order, and every rank receives identical bytes.  With no probes set *count = 0 and
 * DCFM_OK.  After a run that ended in DCFM_ERR_NUMERIC it returns what the device holds (NaN included),
 * as dcfm_get_state_raw.  Errors (DCFM_ERR_INVALID): NULL handle ("null handle"), NULL count
 * ("null argument"). */
int  dcfm_set_probes(dcfm_handle *h, const double *V, int32_t nv, int64_t capacity);
int  dcfm_get_probe_draws(dcfm_handle *h, double *out, int64_t *count);

/* ---- per-sample draws of V' Sigma^{-1} V and log det Sigma (posterior of anything through the inverse) ----
 * dcfm_sigma_solve applies the inverse of the posterior mean.  A Mahalanobis distance, a discriminant
 * score, minimum-variance weights, a partial correlation or the held-out Gaussian log density
 * -(p log 2 pi + log det Sigma(s) + y' Sigma(s)^{-1} y) / 2 need Sigma(s)^{-1} per saved sample.  Sigma(s) =
 * D + rho Lbar Lbar' with D = blockdiag((1 - rho) L_m L_m' + Omega_m) is block-diagonal plus rank K, so two
 * nested Woodbury steps give both from one weighted Gram [L_m V_m]' Omega_m^{-1} [L_m V_m] per shard, g
 * K x K inversions and one more: one read of Lambda, omega and V per saved sample, Sigma(s) never formed, no
 * p x p factorisation and no iteration (csrc/precision.hip has the recursion).
 *
 * dcfm_set_precision_probes: as dcfm_set_probes in every respect not listed here -- V p x nv column-major
 * in Sigmaout's permuted, standardised coordinates, every rank passes the full V and keeps its own rows,
 * recording from the next dcfm_run at every saved sample until `capacity` draws are held, a second call
 * replaces V and resets the count, capacity == 0 turns it off and frees its buffers, nothing allocated or
 * launched until it is on, not collective, booked under DCFM_K_SAVE, no floating-point atomics and fixed
 * summation orders.  Differences: 0 <= nv <= 32, and with nv == 0 (V may be NULL) only log det Sigma(s) is
 * recorded; it is independent of dcfm_set_probes: both may be on at once and neither changes the other's
 * bits.
 * Device bytes: 8 (P g_local nv + capacity * slot + scratch); with w = K + nv and ts = K w + nv^2 + 1 (a
 * term [H | F | q | ld]: H K x K and q nv x nv stored square, one triangle computed and mirrored in q),
 * slot = nv^2 + 1 on one rank (the draw and its log det) and ts on several (the rank's sum of terms), and
 * scratch = g_local s (256 nt + 1) + g_local w^2 + (g_local + ceil(g_local / 8) + 1) ts + K nv doubles: the
 * slice partials (nt = the lower 16 x 16 tiles of w padded to 16, s = min(the probes' s, max(1, P / max(8,
 * wpad / 2))) slices per shard), the shards' Grams, the shard, group and rank terms and one solve, plus a
 * ticket word per shard and group.  The kernel uses up to 8 (K^2 + 16 K) bytes + 2 KiB of LDS (146 KiB at K = 128).
 * Errors (DCFM_ERR_INVALID, a block set before stays as it was): NULL handle ("null handle"), NULL V with
 * capacity > 0 and nv > 0 ("null argument"), nv outside 0..32, capacity < 0, a non-finite entry in V.
 *
 * dcfm_get_precision_draws: count (required) receives the number of draws held; Q (nullable) the nv x nv x
 * count array of V' Sigma(s)^{-1} V in saved-sample order, every slice symmetric bit for bit (one triangle
 * computed, then mirrored); logdet (nullable) the count values of log det Sigma(s).  Blocks (synchronises
 * the sweep stream) and does not disturb a later dcfm_run.  With nothing set *count = 0 and DCFM_OK.  After
 * a run that ended in DCFM_ERR_NUMERIC it returns what the device holds: a NaN state gives NaN draws (the
 * inversions take no data-dependent trip counts).  With nranks > 1 it is collective: every rank's sum
 * [H_r | F_r | q_r | ld_r] of all draws travels in one all-gather, every rank adds them in rank order and
 * closes the K x K step on the host (a plain Cholesky), and every rank receives identical bytes; one rank
 * closes it in the kernel.  Errors (DCFM_ERR_INVALID): NULL handle ("null handle"), NULL count ("null
 * argument"). */
int  dcfm_set_precision_probes(dcfm_handle *h, const double *V, int32_t nv, int64_t capacity);
int  dcfm_get_precision_draws(dcfm_handle *h, double *Q, double *logdet, int64_t *count);

/* ---- pointwise log-likelihood of the training rows per saved sample (WAIC, PSIS-LOO) ----
 * l[s, i] = log N(y_i; 0, Sigma(s)) = -(p log 2 pi + log det Sigma(s) + y_i' Sigma(s)^{-1} y_i) / 2 for every
 * saved sample s and every row i = 1..n of the standardised data the sweep holds (dcfm_get_data), which is what
 * model comparison over g, K and rho needs and no held-out data.  The device records the Mahalanobis part
 * q_i = y_i' Sigma(s)^{-1} y_i and log det Sigma(s) by the recursion of the precision draws with the data rows
 * in the probes' place: one more fp64-MFMA pass over Y per saved sample (T_m = Y_m Omega_m^{-1} Lambda_m, the
 * bytes and MFMAs of the sweep's W pass), the shards' K x K inversions, and n K^2 g flops to close the rows
 * (csrc/loglik.hip has the recursion and the launch chain).
 *
 * dcfm_set_loglik: from the next dcfm_run on every saved sample records one draw until `capacity` draws are
 * held; later saved samples are not recorded; a second call resets the count; capacity == 0 turns it off and
 * frees its buffers; nothing is allocated or launched until a call with capacity > 0.  Not collective.  It needs
 * no data at call time (the data must be set before the run that records).  Booked under DCFM_K_SAVE.  No
 * floating-point atomics and fixed summation orders: the same inputs give the same bits, in one dcfm_run call or
 * one iteration per call.  Independent of dcfm_set_probes and dcfm_set_precision_probes: all three may be on at
 * once and none changes another's bits.
 * Device bytes: 8 (g_local NP (KW + 1) + g_local K^2 + 2 (K^2 + 1) + capacity * slot + scratch), NP = n rounded
 * up to 128 and KW = K padded to 32 / 64 / 128: the pass's T_m and row sums, the shards' B_m^{-1}, the rank's
 * [H | ld] and [S^{-1} | ld]; slot = n + 1 on one rank ([q | ld]) and n K + n + K^2 + 1 on several (the rank's
 * [U_r | q_r | H_r | ld_r]); scratch = that of dcfm_set_precision_probes at nv = 0.  LDS: the Y pass none, the
 * K x K stages up to 8 (K^2 + 16 K) bytes + 2 KiB (the precision draws' kernel), the close 8 ((K + 16) (K | 1) +
 * 272) bytes (147 KiB at K = 128).
 * Errors (DCFM_ERR_INVALID, the setting made before stays as it was): NULL handle ("null handle"), capacity < 0.
 *
 * dcfm_get_loglik: count (required) receives the number of draws held; maha (nullable) the n x count
 * column-major array, q_i of draw s at maha[s * n + i], in saved-sample order and Y's row order (the padding
 * rows of the device layouts never reach it); logdet (nullable) the count values of log det Sigma(s).  Blocks
 * (synchronises the sweep stream) and does not disturb a later dcfm_run.  With nothing set *count = 0 and
 * DCFM_OK.  After a run that ended in DCFM_ERR_NUMERIC it returns what the device holds: a NaN state gives NaN
 * draws (no stage takes a data-dependent trip count).  With nranks > 1 it is collective: every rank's partial
 * of all draws travels in one all-gather, every rank adds them in rank order and closes the K x K step and
 * rho u' S^{-1} u on the host (a plain Cholesky), and every rank receives identical bytes; one rank closes it
 * in the kernel.  Errors (DCFM_ERR_INVALID): NULL handle ("null handle"), NULL count ("null argument"). */
int  dcfm_set_loglik(dcfm_handle *h, int64_t capacity);
int  dcfm_get_loglik(dcfm_handle *h, double *maha, double *logdet, int64_t *count);

/* ---- conditional prediction of unobserved variables (imputation, nowcasting, partly observed held-out rows) ----
 * A new row arrives with the variables of an index set A observed.  Under the posterior, what are the others and
 * how sure are we?  For every saved sample s the device forms, for every variable j and new row t,
 *   yhat_jt(s) = E[(Lambda eta)_j | y_A, Sigma(s)]  (for j outside A this is E[y_j | y_A, Sigma(s)]),
 *   cv_j(s)    = the predictive variance of a fresh observation of variable j given y_A (for j outside A this is
 *                Var[y_j | y_A, Sigma(s)]),
 *   q_t(s) = y_A' Sigma_AA(s)^{-1} y_A  and  log det Sigma_AA(s),
 * and accumulates sum yhat, sum yhat^2 and sum cv over the samples.  Restricting to A only removes rows from the
 * weighted Gram of the precision draws, so Sigma_AA(s) is again block-diagonal plus rank K: the K x K stage is the
 * precision draws' kernel with the weight masked, everything p-sized is one more fp64-MFMA pass over Lambda, and
 * there is no branch on the mask after the Gram (csrc/predict.hip has the recursion and the launch chain).
 * The posterior answer follows by the law of total variance: mean_jt = avg_s yhat_jt(s) and
 * Var[y_j | y_A] = avg_s cv_j(s) + var_s yhat_jt(s) = cvar_j + (m2_jt - mean_jt^2).
 *
 * dcfm_set_predict: Ynew is p x nt column-major in Sigmaout's permuted, standardised coordinates, 0 <= nt <= 32
 * new rows as columns; observed is p bytes, nonzero = observed, one mask for all nt rows.  With nt == 0 (Ynew may
 * be NULL) only cvar and log det Sigma_AA(s) are produced.  Entries of Ynew at unobserved positions are ignored,
 * NaN included (they are masked when copied in, never by a product).  From the next dcfm_run on every saved sample
 * is accumulated and its draw recorded until `capacity` samples are held; later saved samples are ignored, so the
 * accumulators and the draws always cover the same samples.  A second call replaces the inputs and zeroes the
 * accumulators and the count; capacity == 0 turns the feature off and frees its buffers; nothing is allocated or
 * launched until a call with capacity > 0.  Booked under DCFM_K_SAVE.  No floating-point atomics, fixed summation
 * orders, one sample added per launch in sample order: the same inputs give the same bits, in one dcfm_run call
 * or one iteration per call.  Independent of dcfm_set_probes, dcfm_set_precision_probes and dcfm_set_loglik: all
 * may be on at once and none changes another's bits.
 * One rank only: the closing step of Sigma_AA(s) needs the sum over ALL shards of H_m and F_m on the device at
 * save time, one more all-gather per saved sample that the sweep does not have.  On a handle of the collective
 * path (nranks > 1 or DCFM_FLAG_COMM_SELF) a call with capacity > 0 is DCFM_ERR_UNSUPPORTED, whether it comes
 * before or after dcfm_comm_init*, and nothing is set.
 * Device bytes: 8 (P g (3 nt + 1) + K^2 + nt^2 + 1 + g (4 K^2 + 2 K nt) + g K4 (ntp + Kp) + capacity (nt + 1) +
 * scratch) + P g, with K4 = K rounded up to 4, ntp = nt and Kp = K rounded up to 16: the new rows, the three
 * accumulators, S^{-1}, the sample's [q | ld], the K x K products and the coefficients [t_m | I - M_m] of the
 * shards, the draws, the mask; scratch = that of dcfm_set_precision_probes at nv = nt.  LDS: the K x K stages up
 * to 8 (K^2 + 16 K) bytes + 2 KiB (146 KiB at K = 128), the pass over Lambda 256 (K4 + Kp + 2) bytes (66 KiB at K = 128).
 * Errors (DCFM_ERR_INVALID, the setting made before stays as it was): NULL handle ("null handle"), NULL observed
 * with capacity > 0 or NULL Ynew with nt > 0 and capacity > 0 ("null argument"), nt outside 0..32, capacity < 0, a
 * non-finite entry of Ynew at an observed position.
 *
 * dcfm_get_predict: count (required) receives the number of samples accumulated; every other output is nullable.
 * mean and m2 are p x nt column-major: sum yhat / count and sum yhat^2 / count (count is the number of samples
 * actually accumulated, the population form, not effsamp); cvar has p entries, sum cv / count; maha is nt x
 * count column-major, q_t of sample s at maha[s * nt + t]; logdet has count entries.  Blocks (synchronises the
 * sweep stream) and does not disturb a later dcfm_run.  With nothing set *count = 0 and DCFM_OK.  After a run that
 * ended in DCFM_ERR_NUMERIC it returns what the device holds: a NaN state gives NaN outputs (no stage takes a
 * data-dependent trip count).  Errors (DCFM_ERR_INVALID): NULL handle ("null handle"), NULL count ("null
 * argument"). */
int  dcfm_set_predict(dcfm_handle *h, const double *Ynew, const uint8_t *observed, int32_t nt, int64_t capacity);
int  dcfm_get_predict(dcfm_handle *h, double *mean, double *m2, double *cvar, double *maha, double *logdet,
                      int64_t *count);

/* ---- regression of a few variables on all the others: posterior mean and SD of the coefficients ----------------
 * Bayesian factor regression (DCFM_FLAG_REGRESSION at dcfm_create, else DCFM_ERR_INVALID).  The response set is
 * R = (r_1 .. r_q), distinct indices in Sigmaout's permuted, standardised coordinates, O its complement.  Per saved
 * sample s, with Theta(s) = Sigma(s)^-1 of the per-sample matrix of dc:182-192,
 *   T(s) = Theta(s)[:, R]  (p x q),   Q(s) = (T(s)[R, :] + T(s)[R, :]') / 2,
 *   C(s) = Q(s)^-1 = Cov[y_R | y_O, Sigma(s)], the residual covariance (one triangle computed, then mirrored),
 *   B(s) = -T(s) C(s) with the q rows a in R set to exactly 0: E[y_R | y_O, Sigma(s)] = B(s)' y and
 *          B(s)[O, :] = Sigma_OO(s)^-1 Sigma_OR(s), the coefficients of the regression of y_R on y_O,
 *   R2_j(s) = 1 - C(s)_jj / Sigma(s)_{r_j r_j},  Sigma(s)_aa = |Lambda_a(s)|^2 + omega_a(s).
 * The device keeps the sums over the saved samples of B, B.^2 (p x q), C, C.^2 (q x q), R2 and R2.^2 (q).  B(s) is a
 * ratio of entries of Theta(s): its mean is not the ratio of dcfm_get_precision_mean's entries, and it comes with a
 * second moment, hence a per-coefficient posterior SD sqrt(max(0, m2 - mean^2)).  The columns of Theta(s) come from
 * the thin factor panels of the precision mean (Theta(s) is block-diagonal plus low rank): q K-length dot products
 * per row and sample and a q x q Gauss-Jordan inversion per sample, no p x p factorisation.  An entry is accurate
 * to first order in eps cond(Sigma(s)), as the precision mean.  Accumulated at every flush on the assembly stream,
 * one sample at a time in sample order from sums loaded first and stored once; no floating-point atomics, fixed
 * summation orders: the same inputs give the same bits whatever asm_batch is and however the chain is cut into
 * dcfm_run calls.  Booked under DCFM_K_ASSEMBLE.  Independent of every other read-out: none changes another's bits.
 *
 * dcfm_set_regression: resp holds q 0-based indices, 0 <= q <= 32 and q < p.  It takes effect from the next dcfm_run;
 * a second call replaces R and zeroes the accumulators and the count; q == 0 (resp may be NULL) turns the feature off
 * and frees its buffers.  Not collective, but every rank must pass the same resp: every rank holds the gathered
 * panels of all g shards and accumulates all p rows (bitwise equal on all ranks).
 * Device bytes: with the flag, the factor buffer p x 4 round_up(asm_batch K, 16) doubles, the (2 g + 1) asm_batch K^2
 * scratch and the omega slots 2 p asm_batch (all shared with DCFM_FLAG_PRECISION_MEAN / _PARTIAL_CORR); with a
 * response set, 8 (2 p q + 2 (q^2 + q) + asm_batch (q^2 + q + (1 + t) K4 qp)) + 4 (2 q + t + 1 + g), t <= q the shards
 * that hold a response, K4 = K rounded up to 4, qp = q to 16.  LDS: 9.1 KiB static (Q(s) and the inversion's
 * multipliers) in the per-sample kernel, 16.5 KiB static (four 16 x 32 tiles of B(s)) in the pass over the rows.
 * Errors (DCFM_ERR_INVALID, the setting made before stays as it was): NULL handle ("null handle"), the flag not set
 * (the message names DCFM_FLAG_REGRESSION), NULL resp with q > 0 ("null argument"), q outside 0..32 or q >= p, an index
 * outside [0, p), a duplicate index.
 *
 * dcfm_get_regression: count (required) receives the number of samples accumulated; every other output is nullable.
 * coef and coef_m2 are p x q column-major: sum B / count and sum B.^2 / count (count is the number of samples
 * actually accumulated, the population form of dcfm_get_predict, not effsamp), exactly 0 in the rows of R; rcov and
 * rcov_m2 are q x q (symmetric bit for bit), r2 and r2_m2 have q entries.  Blocks (synchronises the sweep and the
 * assembly streams) and does not disturb a later dcfm_run.  With nothing set or no sample accumulated yet *count = 0,
 * DCFM_OK, and nothing else is written.  Not collective: `out` pointers must be non-NULL on every rank that wants the
 * data.  After a run that ended in DCFM_ERR_NUMERIC it returns what the device holds (no stage takes a
 * data-dependent trip count: a NaN runs through).  Errors (DCFM_ERR_INVALID): NULL handle ("null handle"), NULL
 * count ("null argument"). */
int  dcfm_set_regression(dcfm_handle *h, const int64_t *resp, int32_t q);
int  dcfm_get_regression(dcfm_handle *h, double *coef, double *coef_m2, double *rcov, double *rcov_m2, double *r2,
                         double *r2_m2, int64_t *count);

/* ---- missing training data: an on-device imputation step ------------------------------------------------------
 * Given eta, Lambda and ps every missing entry of the training matrix is conditionally independent,
 * Y_ij | . ~ N(eta_i . lambda_j, 1 / ps_j), so one data-augmentation step per Gibbs iteration is a valid extension
 * of the sweep: behind the loading rows of iteration t (X, Z, Lambda, ps of t final, before the sample is saved)
 * the device redraws the missing entries in place in Y and rewrites yy_j = sum_i Y_ij^2 of their columns; every
 * other kernel keeps reading Y as it does without a mask.  For a missing (i, j) of local shard m (global shard mg)
 *   mu = sum_{k < K} eta_ik lambda_jk (k ascending),  eta_ik = sqrt(rho) X_ik + sqrt(1 - rho) Z_mik,
 *   Y_ij = mu + z / sqrt(ps_j),
 * z the standard normal at the Philox counter (site 13, shard mg, row j, normal index i, iteration): the value
 * dcfm_rng_fill_rows(device, cfg.seed, 0, 0, 13, mg, iteration, P, n, P n, out) returns at out[j n + i].  With
 * DCFM_FLAG_INJECT_DRAWS these normals still come from Philox at cfg.seed: dcfm_draws_view keeps its layout and has
 * no member for them.  yy_j is rewritten as yy_obs_j + sum_{i missing} Y_ij^2 in a fixed order, never as an
 * increment of its old value.  The Rao-Blackwellised by-products are, per missing entry, the posterior mean of mu
 * and, by the law of total variance, Var[Y_ij | observed] = nvar_j + m2_ij - mean_ij^2 (csrc/impute.hip has the
 * kernels).
 *
 * dcfm_set_missing: mask_local is n x P x g_local bytes, column-major, the layout of dcfm_set_data's Yd_local;
 * nonzero = missing.  After dcfm_set_data / dcfm_set_data_raw only (else DCFM_ERR_INVALID, "set_data first"); a
 * later dcfm_set_data* turns the feature off, because the mask belongs to the data.  A NULL or all-zero mask turns
 * it off and frees its buffers (yy of the mask's columns then is what dcfm_set_data would form from the completed
 * matrix); nothing is allocated or launched until a call with a missing entry.  Not collective: every rank passes the
 * mask of its own shards, nothing of Y crosses ranks, any number of ranks.  Start values: a missing entry whose
 * current device value is finite keeps it (a completed matrix from dcfm_get_data continues a chain), a non-finite
 * one (the caller passed NaN) becomes 0, the standardised column mean.  yy_obs_j, the sum of squares of column j's
 * observed entries, is formed once here by a direct sum in row order.  `capacity` is the number of saved samples
 * accumulated for dcfm_get_imputed: 0 = draw and rewrite only, no accumulators; later saved samples are ignored;
 * a second call replaces the mask and zeroes the accumulators and the count.  The step runs at every iteration, in
 * both launch schedules and at every K, on the sweep stream, booked under DCFM_K_SAVE.  No floating-point atomics,
 * one sample added per launch in sample order: the same inputs give the same bits, in one dcfm_run call or one
 * iteration per call.
 * Together with dcfm_set_loglik it is DCFM_ERR_UNSUPPORTED, in either call order, and the earlier setting stays:
 * that read-out would be the likelihood of the completed data, not of the observed entries.  More than 2^31 - 1
 * missing entries on a rank: DCFM_ERR_UNSUPPORTED.  A failed call leaves the previous setting as it was.
 * Device bytes: 20 per missing entry + 16 with capacity > 0, and 16 (+ 8) per column with a missing entry.
 * After DCFM_ERR_NUMERIC the imputed entries of Y may be non-finite: dcfm_set_state / dcfm_init_state clear the
 * handle's error as before, and the caller must repeat dcfm_set_data and dcfm_set_missing.  dcfm_get_data returns
 * the completed matrix with the current draw; reading it every few saved samples is multiple imputation.
 * Errors (DCFM_ERR_INVALID): NULL handle ("null handle"), capacity < 0, no data.
 *
 * dcfm_get_imputed: count (required) receives the number of samples accumulated; the other outputs are nullable.
 * mean and m2 are n x P x g_local column-major: at a missing position sum mu / count and sum mu^2 / count (count
 * is the number actually accumulated, the population form), at an observed one Y_ij and Y_ij^2; nvar is P x
 * g_local: sum (1 / ps_j) / count for a column with a missing entry, 0 elsewhere.  Blocks (synchronises the sweep
 * stream), does not disturb a later dcfm_run, not collective.  With nothing set, capacity == 0 or no sample yet:
 * *count = 0, DCFM_OK and the other outputs are not written.  After DCFM_ERR_NUMERIC it returns what the device
 * holds.  Errors (DCFM_ERR_INVALID): NULL handle ("null handle"), NULL count ("null argument"). */
int  dcfm_set_missing(dcfm_handle *h, const uint8_t *mask_local, int64_t capacity);
int  dcfm_get_imputed(dcfm_handle *h, double *mean, double *m2, double *nvar, int64_t *count);

/* ---- measurement --------------------------------------------------------- */
/* Per-kernel HIP-event timing on the handle's stream (off by default).
 * Kernel ids: DCFM_K_* below.  Times are accumulated device milliseconds. */
#define DCFM_K_PREP     0
#define DCFM_K_WPASS    1
#define DCFM_K_ZDRAW    2
#define DCFM_K_XRED     3
#define DCFM_K_XDRAW    4
#define DCFM_K_CPASS    5
#define DCFM_K_LAMBDA   6
#define DCFM_K_COLSUM   7
#define DCFM_K_DELTA    8
#define DCFM_K_SAVE     9
#define DCFM_K_ASSEMBLE 10
#define DCFM_K_COMM     11
#define DCFM_K_XCHOL    12
#define DCFM_K_DRAWS    13   /* on-device Philox variates of the next iteration (side stream) */
#define DCFM_K_RESID    14   /* direct-residual ps / omega (DCFM_FLAG_EXACT_RESIDUAL) */
#define DCFM_K_COUNT    15
int  dcfm_set_profiling(dcfm_handle *h, int enable);
/* Time only the kernels whose bit (1u << DCFM_K_*) is set: two events per timed
 * launch cost host time, so a throughput run times just the kernel it reports. */
int  dcfm_set_profiling_mask(dcfm_handle *h, uint32_t mask);
/* Time one in `stride` launches of each timed kernel (the first of every `stride`; default 1),
 * e.g. to keep event records off most launches of a long run.  Reset to 1 by
 * dcfm_set_profiling[_mask]. */
int  dcfm_set_profiling_stride(dcfm_handle *h, int32_t stride);
int  dcfm_get_kernel_stats(dcfm_handle *h, double ms[DCFM_K_COUNT], int64_t launches[DCFM_K_COUNT]);
const char *dcfm_kernel_name(int id);

/* ---- diagnostics (RNG statistical tests) --------------------------------
 * Fills out[0..count) with on-device Philox variates exactly as the sweep
 * draws them: kind 0 = standard normal, kind 1 = standard gamma(shape).
 * Variate i uses counter (site, shard, row = i / 32, k = i % 32, iter). */
int  dcfm_rng_fill(int device, uint64_t seed, int kind, double shape, int32_t site,
                   int32_t shard, int64_t iter, int64_t count, double *out);
/* As dcfm_rng_fill with rows of `width` variates: out[e], e < count <= rows * width, uses
 * counter (site, shard, row = e / width, k = e % width, iter) — e.g. width = K for the
 * per-row variates of the K > 32 kernels (row j's normals / gammas at indices 0..K-1). */
int  dcfm_rng_fill_rows(int device, uint64_t seed, int kind, double shape, int32_t site,
                        int32_t shard, int64_t iter, int64_t rows, int32_t width, int64_t count,
                        double *out);

#ifdef __cplusplus
}
#endif
#endif /* DCFM_H */
