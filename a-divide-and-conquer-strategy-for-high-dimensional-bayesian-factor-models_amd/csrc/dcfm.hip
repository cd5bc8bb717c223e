// C-ABI implementation (include/dcfm.h): creating and destroying a handle with its HBM
// allocation, and the per-iteration launch sequence of the hot loop (divideconquer.m:90-197)
// in its two layouts.  Collectives: comm.hip; data and state I/O: state_io.hip; the Sigma
// read-out: sigma_out.hip.
#include "handle.h"
#include "resid.h"   // KAPPA_IDENTITY_MAX

static int dalloc(dcfm_handle *h, double **p, size_t n) {
    void *q = nullptr;
    if (n == 0) n = 1;
    hipError_t e = hipMalloc(&q, n * sizeof(double));
    if (e != hipSuccess)
        return fail(h, DCFM_ERR_ALLOC, "hipMalloc(%zu doubles) failed: %s", n, hipGetErrorString(e));
    e = hipMemset(q, 0, n * sizeof(double));
    if (e != hipSuccess) return fail(h, DCFM_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(e));
    h->allocs.push_back(q);
    *p = static_cast<double *>(q);
    return DCFM_OK;
}

static int round_up(int a, int b) { return (a + b - 1) / b * b; }

// row t of the chain trace ([G][4] shard sums after the scratch, trace.hip)
static double *trace_row(dcfm_handle *h, int64_t t) {
    return h->trace + trace_scratch_doubles(h->d.G) + (size_t)t * h->d.G * 4;
}

static void collect_prof(dcfm_handle *h) {
    if (h->recs.empty()) return;
    sync_all(h);
    for (auto &r : h->recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            h->kms[r.kid] += ms;
            h->kcnt[r.kid] += 1;
        }
        h->evpool.push_back(r.a);
        h->evpool.push_back(r.b);
    }
    h->recs.clear();
}

// Sigma block-sharding: tile rows [Tb[k], Tb[k+1]) to rank k, contiguous, each rank's
// share of the nt(nt+1)/2 lower tiles as near total/nranks as row granularity allows
// (rank k's tiles: tri(Tb[k+1]) - tri(Tb[k])).  Ranks may own no rows when nt < nranks.
static std::vector<int> sigma_split(int nt, int nranks) {
    std::vector<int> Tb(nranks + 1, nt);
    Tb[0] = 0;
    const double total = (double)tri(nt);
    for (int k = 1; k < nranks; ++k) {
        const double target = total * k / nranks;
        int t = Tb[k - 1];
        while (t < nt && (double)tri(t) < target) ++t;                 // first t with tri(t) >= target
        if (t > Tb[k - 1] && target - (double)tri(t - 1) < (double)tri(t) - target) --t;   // the nearer
        Tb[k] = t;
    }
    return Tb;
}

// ---------------------------------------------------------------------------
extern "C" {

int dcfm_abi_version(void) { return DCFM_ABI_VERSION; }

const char *dcfm_last_error(const dcfm_handle *h) { return h ? h->err.c_str() : g_err.c_str(); }

const char *dcfm_kernel_name(int id) {
    static const char *names[DCFM_K_COUNT] = {"k_prep",  "k_wpass", "k_zdraw",  "k_xred",
                                              "k_xdraw", "k_cpass", "k_lambda", "k_colsum",
                                              "k_delta", "k_save",  "k_assemble", "rccl", "k_xchol",
                                              "k_draws", "k_resid"};
    return (id >= 0 && id < DCFM_K_COUNT) ? names[id] : "?";
}

// dcfm_create's checks of the configuration, before any device is touched
static int validate_config(const dcfm_config &c) {
    if (c.n < 1 || c.P < 1 || c.g < 1 || c.K < 1)
        return fail(nullptr, DCFM_ERR_INVALID, "n, P, g, K must be >= 1");
    if (c.K > KP_MAX)
        return fail(nullptr, DCFM_ERR_UNSUPPORTED, "K = %d > %d not supported by this build", c.K, KP_MAX);
    if (!(c.rho >= 0.0 && c.rho <= 1.0)) return fail(nullptr, DCFM_ERR_INVALID, "rho must be in [0,1]");
    if (c.thin < 1 || c.mcmc < 0 || c.burnin < 0)
        return fail(nullptr, DCFM_ERR_INVALID, "thin >= 1, mcmc >= 0, burnin >= 0 required");
    if (!(c.bs > 0 && c.bd1 > 0 && c.bd2 > 0 && c.df > 0))
        return fail(nullptr, DCFM_ERR_INVALID, "bs, bd1, bd2, df must be > 0 (dc:62-65)");
    // on-device gammas (philox.h): Marsaglia-Tsang for shape >= 1, boosted below 1, so every
    // positive hyper-parameter the reference accepts (dc:62-65) is drawn on the device
    if (!(c.as_ > 0.0 && c.ad1 > 0.0 && c.ad2 > 0.0))
        return fail(nullptr, DCFM_ERR_INVALID, "as, ad1, ad2 must be > 0 (dc:62-65; got %g, %g, %g)", c.as_, c.ad1,
                    c.ad2);
    const int nranks = c.nranks < 1 ? 1 : c.nranks;
    if (c.rank < 0 || c.rank >= nranks) return fail(nullptr, DCFM_ERR_INVALID, "bad rank");
    {   // the fused K <= 32 chain keeps the canonical shard-sum trees' levels in registers
        // (k_wcol TreeSum<.., 8>, k_xdraw <.., 10>); the other layouts sum with TREE_LEVELS = 16
        const bool fused = c.K <= KP && !(c.flags & DCFM_FLAG_UNFUSED);
        const int Gl = c.g / nranks, nxs = xsum_blocks(Gl);
        if (fused && (c.g > 1023 || nxs > 255 || Gl / nxs > 255))
            return fail(nullptr, DCFM_ERR_UNSUPPORTED, "g = %d shards (%d per rank): the fused K <= 32 chain takes at "
                        "most 1023, and a per-rank count whose odd part is below 256 (DCFM_FLAG_UNFUSED lifts "
                        "this)", c.g, Gl);
        if (!fused && c.g >= (1 << 16))    // TreeSum's default depth (linalg.h TREE_LEVELS)
            return fail(nullptr, DCFM_ERR_UNSUPPORTED, "g = %d shards: at most %d", c.g, (1 << 16) - 1);
    }
    if (c.g % nranks)
        return fail(nullptr, DCFM_ERR_UNSUPPORTED, "g = %d not divisible by nranks = %d", c.g, nranks);
    return DCFM_OK;
}

// Everything dcfm_create derives from a valid configuration by host arithmetic (no HIP call): the
// dimensions, the launch layout, the saved samples per assembly batch and the row stride of Lb
static Dims plan(const dcfm_config &c, bool *fused, int *B, int *LDB) {
    Dims d{};
    const int nranks = c.nranks < 1 ? 1 : c.nranks;
    d.n = c.n; d.P = c.P; d.g = c.g; d.K = c.K;
    d.nranks = nranks; d.rank = c.rank;
    d.coll = (nranks > 1 || (c.flags & DCFM_FLAG_COMM_SELF)) ? 1 : 0;
    d.G = c.g / nranks;
    d.shard0 = c.rank * d.G;
    d.NP = round_up(c.n, 128);
    d.PP = round_up(c.P, 32);
    d.p = c.P * c.g;
    d.kp = padded_width(c.K);
    d.rho = c.rho; d.sr = std::sqrt(c.rho); d.s1r = std::sqrt(1.0 - c.rho);
    d.as_ = c.as_; d.bs = c.bs; d.df = c.df; d.ad1 = c.ad1; d.bd1 = c.bd1; d.ad2 = c.ad2; d.bd2 = c.bd2;
    d.seed = c.seed;
    d.inject = (c.flags & DCFM_FLAG_INJECT_DRAWS) ? 1 : 0;
    // K <= 32 runs the fused launch chain unless DCFM_FLAG_UNFUSED asks for the side-stream layout
    *fused = d.kp == KP && !(c.flags & DCFM_FLAG_UNFUSED);
    // fused narrow chain on several ranks: column sums, the A sum and the X message travel in
    // ONE message per iteration (Dims::sgap / xstride)
    const bool packed = d.coll && *fused;
    d.sgap = packed ? KP * KP + d.NP * KP : 0;
    d.xstride = packed ? d.G * KP + KP * KP + d.NP * KP : d.kp * d.kp;
    *B = c.asm_batch > 0 ? c.asm_batch : 32;
    *LDB = round_up(*B * d.K, ASM_KC);
    return d;
}

static int create_streams_and_events(dcfm_handle *h) {
    const dcfm_config &c = h->cfg;
    HIPC(h, hipSetDevice(c.device));
    // Stream priorities: the sweep chain (main, side) at the greatest priority, the draws
    // a batch ahead and the covariance assembly at the least, so the dispatcher hands
    // freed CUs to the latency-critical chain first (DCFM_FLAG_FLAT_PRIORITY: all default).
    int prio_lo = 0, prio_hi = 0;
    if (!(c.flags & DCFM_FLAG_FLAT_PRIORITY)) HIPC(h, hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    HIPC(h, hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, prio_hi));
    {   // DCFM_FLAG_ONE_STREAM: one stream for everything (isolated per-kernel timings)
        if (c.flags & DCFM_FLAG_ONE_STREAM) {
            h->side = h->sasm = h->sdraw = h->stream;
        } else {
            HIPC(h, hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, prio_hi));
            HIPC(h, hipStreamCreateWithPriority(&h->sdraw, hipStreamNonBlocking, prio_lo));
            HIPC(h, hipStreamCreateWithPriority(&h->sasm, hipStreamNonBlocking, prio_lo));
        }
    }
    for (hipEvent_t *e : {&h->e_lam, &h->e_prep, &h->e_xchol, &h->e_batch, &h->e_free[0], &h->e_free[1], &h->e_drawn[0],
                          &h->e_used[0], &h->e_drawn[1], &h->e_used[1]})
        HIPC(h, hipEventCreateWithFlags(e, hipEventDisableTiming));
    return DCFM_OK;
}

// the non-finite sentinel, then every device buffer of h->d's layout (zeroed)
static int alloc_buffers(dcfm_handle *h) {
    const dcfm_config &c = h->cfg;
    const int nranks = c.nranks;
    void *q = nullptr;
    HIPC(h, hipMalloc(&q, sizeof(int)));
    h->allocs.push_back(q);
    h->nan_dev = static_cast<int *>(q);
    HIPC(h, hipMemset(h->nan_dev, 0, sizeof(int)));
    HIPC(h, hipHostMalloc(&q, sizeof(int), hipHostMallocDefault));
    h->nan_host = static_cast<int *>(q);
    *h->nan_host = 0;
    const Dims &d = h->d;
    Bufs &b = h->b;
    const size_t G = d.G, NP = d.NP, PP = d.PP, g = d.g, p = d.p, KP = d.kp;
    TRY(dalloc(h, &b.Y, G * NP * PP));
    TRY(dalloc(h, &b.yy, G * PP));
    TRY(dalloc(h, &b.Lam, G * PP * KP));
    TRY(dalloc(h, &b.omega, G * PP));
    TRY(dalloc(h, &b.ps, G * PP));
    TRY(dalloc(h, &b.psi, G * PP * KP));
    TRY(dalloc(h, &b.Plam, G * PP * KP));
    TRY(dalloc(h, &b.X, NP * KP));
    TRY(dalloc(h, &b.Z, G * NP * KP));
    TRY(dalloc(h, &b.delta, 2 * g * KP));
    TRY(dalloc(h, &b.tau, 2 * g * KP));
    TRY(dalloc(h, &b.W, G * NP * KP));
    TRY(dalloc(h, &b.A, G * KP * KP));
    TRY(dalloc(h, &b.ZM, G * 4 * KP * KP));
    TRY(dalloc(h, &b.Sp, G * NP * KP));
    if (d.sgap) {   // packed message [sloc | xa | xin] and its gather (dcfm_internal.h, Dims::sgap)
        const size_t msg = (size_t)d.xstride;
        TRY(dalloc(h, &b.sloc, msg));
        b.xa = b.sloc + (size_t)G * KP;
        b.xin = b.xa + KP * KP;
        TRY(dalloc(h, &b.msg_all, (size_t)nranks * msg));
        b.sall = b.msg_all;
        b.xa_all = b.msg_all + (size_t)G * KP;
        b.xall = b.xa_all + KP * KP;
    } else {
        TRY(dalloc(h, &b.xin, NP * KP));
        if (d.coll) { TRY(dalloc(h, &b.xall, (size_t)nranks * NP * KP)); } else b.xall = b.xin;
        TRY(dalloc(h, &b.xa, KP * KP));
        TRY(dalloc(h, &b.xa_all, (size_t)nranks * KP * KP));
    }
    TRY(dalloc(h, &b.XM, 2 * KP * KP));
    TRY(dalloc(h, &b.agree, 3));
    {
        double *rf = nullptr;
        TRY(dalloc(h, &rf, (G * (PP / 32) + 1) / 2));   // zeroed: no tile flagged
        b.rflag = reinterpret_cast<int *>(rf);
    }
    TRY(dalloc(h, &b.xpart, (size_t)G * KP * KP));  // k_wcol: xsum_blocks(G) <= G chunk sums
    {
        double *tk = nullptr;
        TRY(dalloc(h, &tk, 1));
        b.ticket = reinterpret_cast<unsigned *>(tk);
        double *sy = nullptr;
        TRY(dalloc(h, &sy, SYNC_ZM + G));           // zeroed: the hand-off counters start at 0 (<= 255 chunks, G shards)
        b.sync = reinterpret_cast<unsigned long long *>(sy);
    }
    TRY(dalloc(h, &b.C, G * PP * KP));
    TRY(dalloc(h, &b.E, G * KP * KP));
    TRY(dalloc(h, &b.cpart, G * PP * KP));
    if (!d.sgap) {
        TRY(dalloc(h, &b.sloc, G * KP));
        if (d.coll) { TRY(dalloc(h, &b.sall, g * KP)); } else b.sall = b.sloc;
    }
    TRY(dalloc(h, &b.Lb[0], p * (size_t)b.LDB));
    TRY(dalloc(h, &b.Lb[1], p * (size_t)b.LDB));
    TRY(dalloc(h, &b.wsum[0], p));
    TRY(dalloc(h, &b.wsum[1], p));
    // Sigmaout block-sharded over ranks: contiguous tile rows balanced by tile count
    {
        const int nt = (d.p + ASM_TILE - 1) / ASM_TILE;
        h->Tb = sigma_split(nt, nranks);
        b.T0 = h->Tb[c.rank];
        b.T1 = h->Tb[c.rank + 1];
    }
    TRY(dalloc(h, &b.Sigma, (size_t)(tri(b.T1) - tri(b.T0)) * ASM_TILE * ASM_TILE));
    if (c.flags & DCFM_FLAG_SIGMA_M2) {   // second moment beside the mean, and each saved sample's own omega
        TRY(dalloc(h, &b.Sigma2, (size_t)(tri(b.T1) - tri(b.T0)) * ASM_TILE * ASM_TILE));
    }
    if (c.flags & DCFM_FLAG_PRECISION_MEAN)     // mean of the per-sample inverse
        TRY(dalloc(h, &h->pm.Prec, (size_t)(tri(b.T1) - tri(b.T0)) * ASM_TILE * ASM_TILE));
    if (c.flags & DCFM_FLAG_PARTIAL_CORR) {     // mean and second moment of the per-sample partial correlations
        TRY(dalloc(h, &h->pc.PC, (size_t)(tri(b.T1) - tri(b.T0)) * ASM_TILE * ASM_TILE));
        TRY(dalloc(h, &h->pc.PC2, (size_t)(tri(b.T1) - tri(b.T0)) * ASM_TILE * ASM_TILE));
    }
    // their factor panels and K x K scratch; DCFM_FLAG_REGRESSION reads the same panels (regression.hip)
    if (c.flags & (DCFM_FLAG_PRECISION_MEAN | DCFM_FLAG_PARTIAL_CORR | DCFM_FLAG_REGRESSION)) {
        PrecMean &pm = h->pm;
        pm.KH = round_up(h->B * d.K, ASM_KC);
        TRY(dalloc(h, &pm.pfac, p * 4 * (size_t)pm.KH));
        TRY(dalloc(h, &pm.pscr, precision_mean_scratch_doubles(d.g, d.K, h->B)));
        HIPC(h, precision_mean_setup());
    }
    if (c.flags & DCFM_FLAG_CORR) {             // mean and second moment of the per-sample correlations and communalities
        Corr &cr = h->cr;
        TRY(dalloc(h, &cr.C, (size_t)(tri(b.T1) - tri(b.T0)) * ASM_TILE * ASM_TILE));
        TRY(dalloc(h, &cr.C2, (size_t)(tri(b.T1) - tri(b.T0)) * ASM_TILE * ASM_TILE));
        TRY(dalloc(h, &cr.cscale, p * (size_t)h->B));
        TRY(dalloc(h, &cr.H, p));
        TRY(dalloc(h, &cr.H2, p));
    }
    if (c.flags & (DCFM_FLAG_SIGMA_M2 | DCFM_FLAG_PRECISION_MEAN | DCFM_FLAG_PARTIAL_CORR | DCFM_FLAG_CORR |
                   DCFM_FLAG_REGRESSION)) {   // each saved sample's own omega
        TRY(dalloc(h, &b.wslot[0], p * (size_t)h->B));
        TRY(dalloc(h, &b.wslot[1], p * (size_t)h->B));
    }
    // the generated fused chain: k_wcol's LAMGEN blocks draw the loading-row variates into b.ldraw
    // each iteration (lam_draws)
    if (h->fused && !d.inject) TRY(dalloc(h, &b.ldraw, (size_t)lam_gen_doubles(d)));
    if (!d.inject && !h->fused) {   // k_draws batches of the side-stream layouts
        const size_t K = c.K, n = c.n, P = c.P;
        const size_t nz = K * n * g, nx = K * n, nl = K * P * g, gpsi = P * K * g, gdel = K * g, gps = P * g;
        const size_t per_it = nz + nx + nl + gpsi + gdel + gps;
        // batches of up to 8 iterations, two slots within ~2 GiB
        h->DB = (int)std::max<size_t>(1, std::min<size_t>(8, (size_t(2) << 30) / (2 * per_it * sizeof(double))));
        const size_t sz[6] = {nz, nx, nl, gpsi, gdel, gps};
        for (int i = 0; i < 6; ++i) h->draw_iter_sz[i] = sz[i];
        double *gm = nullptr;
        TRY(dalloc(h, &gm, 2 * (size_t)h->DB * per_it));
        for (int sl = 0; sl < 2; ++sl) {
            DrawsDev &G = h->gen[sl];
            G.NZ = gm; gm += nz * h->DB;
            G.NX = gm; gm += nx * h->DB;
            G.NL = gm; gm += nl * h->DB;
            G.Gpsi = gm; gm += gpsi * h->DB;
            G.Gdelta = gm; gm += gdel * h->DB;
            G.Gps = gm; gm += gps * h->DB;
            G.first_iter = -1;
            G.n_iter = h->DB;
        }
    }
    return DCFM_OK;
}

// this rank's lower-triangle assembly tiles in k_assemble's processing order: 8 x 8-tile
// supertiles (row bands of the rank's block, then column bands), row-major inside — the
// tiles an XCD runs together share their Lb panels in L2.  (Storage is by (ti, tj).)
static int upload_tile_list(dcfm_handle *h) {
    Bufs &b = h->b;
    constexpr int SB = 8;
    std::vector<int2> tl;
    for (int rb0 = b.T0; rb0 < b.T1; rb0 += SB) {
        const int rb1 = std::min(b.T1, rb0 + SB);
        for (int cb0 = 0; cb0 < rb1; cb0 += SB)
            for (int ti = rb0; ti < rb1; ++ti)
                for (int tj = cb0; tj < std::min(cb0 + SB, ti + 1); ++tj) tl.push_back(make_int2(ti, tj));
    }
    if ((int64_t)tl.size() != tri(b.T1) - tri(b.T0))
        return fail(h, DCFM_ERR_INVALID, "assembly tile list: %zu tiles for %lld", tl.size(),
                    (long long)(tri(b.T1) - tri(b.T0)));
    b.ntiles = (int)tl.size();
    void *q = nullptr;
    HIPC(h, hipMalloc(&q, std::max<size_t>(1, tl.size()) * sizeof(int2)));
    h->allocs.push_back(q);
    b.tiles = static_cast<int2 *>(q);
    if (!tl.empty()) HIPC(h, hipMemcpy(b.tiles, tl.data(), tl.size() * sizeof(int2), hipMemcpyHostToDevice));
    return DCFM_OK;
}

// pad delta/tau with ones
static int fill_delta_tau_ones(dcfm_handle *h) {
    std::vector<double> ones(2 * (size_t)h->d.g * h->d.kp, 1.0);
    HIPC(h, hipMemcpy(h->b.delta, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPC(h, hipMemcpy(h->b.tau, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
    return DCFM_OK;
}

int dcfm_create(const dcfm_config *cfg, dcfm_handle **out) {
    if (!cfg || !out) return fail(nullptr, DCFM_ERR_INVALID, "null argument");
    *out = nullptr;
    const dcfm_config &c = *cfg;
    TRY(validate_config(c));
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(nullptr, DCFM_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
    if (c.device < 0 || c.device >= ndev) return fail(nullptr, DCFM_ERR_INVALID, "bad device %d", c.device);

    dcfm_handle *h = new dcfm_handle();
    h->d = plan(c, &h->fused, &h->B, &h->b.LDB);
    h->cfg = c;
    h->cfg.nranks = h->d.nranks;
    int rc = create_streams_and_events(h);
    if (rc == DCFM_OK) rc = alloc_buffers(h);
    if (rc == DCFM_OK) rc = upload_tile_list(h);
    if (rc == DCFM_OK) rc = fill_delta_tau_ones(h);
    if (rc != DCFM_OK) {   // the one failure path: the message outlives the handle in g_err
        g_err = h->err;
        dcfm_destroy(h);
        return rc;
    }
    *out = h;
    return DCFM_OK;
}

void dcfm_destroy(dcfm_handle *h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) sync_all(h);
    for (auto &r : h->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : h->evpool) (void)hipEventDestroy(e);
    for (hipEvent_t e : {h->e_lam, h->e_prep, h->e_xchol, h->e_batch, h->e_free[0], h->e_free[1], h->e_drawn[0],
                         h->e_drawn[1], h->e_used[0], h->e_used[1]})
        if (e) (void)hipEventDestroy(e);
    if (h->lp_ready) (void)hipEventDestroy(h->lp_ready);
    if (h->lp_done) (void)hipEventDestroy(h->lp_done);
    if (h->comm_asm) ncclCommDestroy(h->comm_asm);
    if (h->comm_side) ncclCommDestroy(h->comm_side);
    if (h->comm) ncclCommDestroy(h->comm);
    for (void *q : h->allocs) (void)hipFree(q);
    if (h->nan_host) (void)hipHostFree(h->nan_host);
    if (h->draws_mem) (void)hipFree(h->draws_mem);
    if (h->trace) (void)hipFree(h->trace);
    if (h->probe_mem) (void)hipFree(h->probe_mem);
    if (h->prec_mem) (void)hipFree(h->prec_mem);
    if (h->ll_mem) (void)hipFree(h->ll_mem);
    if (h->pred_mem) (void)hipFree(h->pred_mem);
    if (h->imp_mem) (void)hipFree(h->imp_mem);
    if (h->reg_mem) (void)hipFree(h->reg_mem);
    if (h->sasm && h->sasm != h->stream) (void)hipStreamDestroy(h->sasm);
    if (h->side && h->side != h->stream) (void)hipStreamDestroy(h->side);
    if (h->sdraw && h->sdraw != h->stream) (void)hipStreamDestroy(h->sdraw);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// Hand the filled Lb[lb] batch to the assembly stream (overlaps the next iterations).
static int flush_batch(dcfm_handle *h) {
    if (h->batch == 0) return DCFM_OK;
    Dims &d = h->d;
    Bufs &b = h->b;
    const int lb = h->lb;
    HIPC(h, hipEventRecord(h->e_batch, h->stream));
    HIPC(h, hipStreamWaitEvent(h->sasm, h->e_batch, 0));
    if (d.coll) {
        KTimer t(h, DCFM_K_COMM, h->sasm);
        const size_t rows = (size_t)d.G * d.P;
        if (!h->loop) NCCLC(h, ncclGroupStart());
        int rc = coll_allgather(h, CH_ASM, b.Lb[lb] + (size_t)d.rank * rows * b.LDB, b.Lb[lb], rows * b.LDB,
                                h->sasm);
        if (rc == DCFM_OK)
            rc = coll_allgather(h, CH_ASM, b.wsum[lb] + (size_t)d.rank * rows, b.wsum[lb], rows, h->sasm);
        if (rc == DCFM_OK && b.wslot[lb])
            rc = coll_allgather(h, CH_ASM, b.wslot[lb] + (size_t)d.rank * rows * h->B, b.wslot[lb], rows * h->B,
                                h->sasm);
        if (!h->loop) NCCLC(h, ncclGroupEnd());
        if (rc) return rc;
    }
    // k extent: the batch's columns rounded to the MFMA k-step (4); k_assemble stages whole
    // chunks of ASM_KC columns, so columns [used, round_up(used, ASM_KC)) must be zero
    const int used = h->batch * d.K, kext = round_up(used, 4), kstage = round_up(used, ASM_KC);
    const double effsamp = (double)h->cfg.mcmc / (double)h->cfg.thin;   // dc:45 (Q8)
    // k_save wrote columns [0, used) of every row; only the chunk's tail [used, kstage) can
    // hold an earlier batch's samples: zero just that (not the p x LDB buffer)
    if (kstage > used)
        HIPC(h, hipMemset2DAsync(b.Lb[lb] + used, (size_t)b.LDB * sizeof(double), 0, (size_t)(kstage - used) * sizeof(double),
                                 (size_t)d.p, h->sasm));
    {
        KTimer t(h, DCFM_K_ASSEMBLE, h->sasm);
        launch_assemble(d, b, b.Lb[lb], b.wsum[lb], kext, 1.0 / effsamp, h->sasm);
        // DCFM_FLAG_SIGMA_M2: the batch's samples one by one into the second moment
        if (b.Sigma2) launch_assemble_m2(d, b, b.Lb[lb], b.wslot[lb], h->batch, h->B, 1.0 / effsamp, h->sasm);
        // the factor panels of the batch's per-sample inverses, once for all of their readers
        if (h->pm.pfac && (h->pm.Prec || h->pc.PC || h->rg.q)) launch_precision_panels(d, b, h->pm, b.Lb[lb], b.wslot[lb], h->batch, h->B, h->sasm);
        // DCFM_FLAG_PRECISION_MEAN: the inverses into the precision mean
        if (h->pm.Prec) launch_precision_mean(d, b, h->pm, b.wslot[lb], h->batch, h->B, 1.0 / effsamp, h->sasm);
        // dcfm_set_regression: the coefficients of the batch's samples, from the panels as the panel stage left them
        if (h->rg.q) {
            launch_regression(d, b, h->pm, h->rg, b.Lb[lb], b.wslot[lb], h->batch, h->B, h->sasm);
            h->reg_n += h->batch;
        }
        // DCFM_FLAG_PARTIAL_CORR: the panels scaled in place, the partial correlations into their two moments
        if (h->pc.PC) launch_partial_corr(d, b, h->pm, h->pc, b.wslot[lb], h->batch, h->B, 1.0 / effsamp, h->sasm);
        // DCFM_FLAG_CORR: the rows' scales and communalities, the per-sample correlations into their two moments
        if (h->cr.C) launch_corr(d, b, h->cr, b.Lb[lb], b.wslot[lb], h->batch, h->B, 1.0 / effsamp, h->sasm);
    }
    HIPC(h, hipGetLastError());
    HIPC(h, hipMemsetAsync(b.wsum[lb], 0, (size_t)d.p * sizeof(double), h->sasm));   // k_save adds into it
    HIPC(h, hipEventRecord(h->e_free[lb], h->sasm));
    h->asm_pending[lb] = true;
    h->lb ^= 1;
    h->batch = 0;
    return DCFM_OK;
}

// dcfm_run: two launch schedules, fixed at create (h->fused: FusedSchedule, else SideSchedule),
// which share the loading-row launch, "iteration complete" and the sample save
static int check_run_args(dcfm_handle *h, int64_t first_iter, int64_t n_iter) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    if (!h->have_data || !h->have_state) return fail(h, DCFM_ERR_INVALID, "set_data and set_state first");
    if (first_iter < 1 || n_iter < 0) return fail(h, DCFM_ERR_INVALID, "iterations are 1-based");
    if (h->d.coll && !h->comm_ok) return fail(h, DCFM_ERR_INVALID, "dcfm_comm_init first (nranks > 1 or COMM_SELF)");
    if (h->d.inject) {
        if (!h->dr.NZ) return fail(h, DCFM_ERR_INVALID, "INJECT_DRAWS set but no draws");
        if (first_iter < h->dr.first_iter || first_iter + n_iter > h->dr.first_iter + h->dr.n_iter)
            return fail(h, DCFM_ERR_INVALID, "iterations [%lld,%lld) not covered by injected draws",
                        (long long)first_iter, (long long)(first_iter + n_iter));
    }
    return DCFM_OK;
}

// the double-buffered delta / tau: h->cur is the buffer in use, the chain writes the other
struct DeltaTau { const double *delta_in, *tau_in; double *delta_out, *tau_out; };
static DeltaTau delta_tau(const dcfm_handle *h) {
    const size_t nkg = (size_t)h->d.g * h->d.kp, in = h->cur * nkg, out = (1 - h->cur) * nkg;
    return {h->b.delta + in, h->b.tau + in, h->b.delta + out, h->b.tau + out};
}

// an iteration's delta chain is queued: its tau becomes the current one
static void iteration_done(dcfm_handle *h) {
    h->cur ^= 1;
    if (h->trace_n < h->trace_cap) {                                  // dcfm_set_trace
        launch_trace(h->d, h->b, delta_tau(h).tau_in, h->trace, trace_row(h, h->trace_n), h->stream);
        h->trace_n += 1;
    }
}

// dc:180: is iteration it's sample saved?
static bool saved_iteration(const dcfm_handle *h, int64_t it) { return it % h->cfg.thin == 0 && it > h->cfg.burnin; }

// Who saves it: k_lambda itself (K <= 32: the row's Lambda and omega are in its registers), unless omega is
// rewritten after it (DCFM_FLAG_EXACT_RESIDUAL: k_resid); then, and for K > 32, k_save copies Lam and omega
#ifndef DCFM_LAM_SAVE
#define DCFM_LAM_SAVE 1   // 0: the A/B baseline, k_save always
#endif
static bool lambda_saves(const dcfm_handle *h) {
    return DCFM_LAM_SAVE && h->d.kp == KP && !(h->cfg.flags & DCFM_FLAG_EXACT_RESIDUAL);
}

// before the first writer of a sample into the open batch: a buffer that is still being assembled
static int open_batch(dcfm_handle *h) {
    if (h->batch == 0 && h->asm_pending[h->lb]) {
        HIPC(h, hipStreamWaitEvent(h->stream, h->e_free[h->lb], 0));
        h->asm_pending[h->lb] = false;
    }
    return DCFM_OK;
}

// the loading rows (k_lambda) and dc:169's direct residual where it is asked for, then the imputation step of
// dcfm_set_missing (the iteration's X, Z, Lambda and ps are final behind them).  Launch chain of a
// saved iteration, K <= 32: [wait e_free of a batch's first sample] k_lambda (writes the sample into
// slot h->batch of Lb / wsum / wslot [h->lb]) -> save_sample: probes, the batch count, the flush of a full
// batch behind it.  Exact residual and K > 32: k_lambda, k_resid / k_resid_flagged, then k_save.
static int loading_rows(dcfm_handle *h, const DrawsDev &dr, int64_t it, bool lamgen) {
    const Dims &d = h->d;
    const Bufs &b = h->b;
    hipStream_t s = h->stream;
    // exact residual: k_resid redoes every row below (the guard need not fire); GUARD_ALL: it rejects every row
    const bool exact = h->cfg.flags & DCFM_FLAG_EXACT_RESIDUAL;
    const double kappa_max = exact ? HUGE_VAL : (h->cfg.flags & DCFM_FLAG_GUARD_ALL) ? 0.0 : KAPPA_IDENTITY_MAX;
    SaveArgs sv;
    if (lambda_saves(h) && saved_iteration(h, it)) {
        TRY(open_batch(h));
        sv.Lb = b.Lb[h->lb]; sv.wsum = b.wsum[h->lb]; sv.wslot = b.wslot[h->lb];
        sv.LDB = b.LDB; sv.slot = h->batch; sv.B = h->B;
    }
    {
        KTimer t(h, DCFM_K_LAMBDA, s);
        launch_lambda(d, b, dr, it, delta_tau(h).tau_in, h->plam_valid ? b.Plam : nullptr, s, lamgen, kappa_max, sv);
    }
    if (exact) {                                      // dc:169's residual for every loading row
        KTimer t(h, DCFM_K_RESID, s);
        launch_resid(d, b, dr, it, s, lamgen);
    } else if (d.kp != KP) {                          // K > 32: the tiles k_lambda_w's guard flagged
        KTimer t(h, DCFM_K_RESID, s);
        launch_resid_flagged(d, b, dr, it, s);
    }
    h->plam_valid = false;
    if (h->imp.nmiss) {                               // dcfm_set_missing: X, Z, Lambda, ps of it are final
        KTimer t(h, DCFM_K_SAVE, s);
        const bool acc = saved_iteration(h, it) && h->imp_n < h->imp_cap;
        launch_impute(d, b, h->imp, it, acc, s);
        if (acc) h->imp_n += 1;
    }
    return DCFM_OK;
}

// dc:180: iteration it's sample is in the open assembly batch (k_lambda wrote it) or goes there now
// (k_save); a full batch is handed over
static int save_sample(dcfm_handle *h, int64_t it) {
    if (!saved_iteration(h, it)) return DCFM_OK;
    const Bufs &b = h->b;
    hipStream_t s = h->stream;
    const bool ksave = !lambda_saves(h);
    if (ksave) TRY(open_batch(h));
    if (ksave || h->probe_n < h->probe_cap || h->prec_n < h->prec_cap || h->ll_n < h->ll_cap ||
        h->pred_n < h->pred_cap) {
        KTimer t(h, DCFM_K_SAVE, s);
        if (ksave) launch_save(h->d, b, b.Lb[h->lb], b.wsum[h->lb], h->batch, s, b.wslot[h->lb], h->B);
        if (h->probe_n < h->probe_cap) launch_probes(h->d, b, h->probes, h->probe_n++, s);   // dcfm_set_probes
        if (h->prec_n < h->prec_cap) launch_precision(h->d, b, h->prec, h->prec_n++, s);   // dcfm_set_precision_probes
        if (h->ll_n < h->ll_cap) launch_loglik(h->d, b, h->ll, h->ll_n++, s);               // dcfm_set_loglik
        if (h->pred_n < h->pred_cap) launch_predict(h->d, b, h->pred, h->pred_n++, s);      // dcfm_set_predict
    }
    HIPC(h, hipGetLastError());
    h->batch += 1;
    h->saved += 1;
    if (h->batch == h->B) TRY(flush_batch(h));
    return DCFM_OK;
}

// Fused schedule (K <= 32), everything on the main stream.  Per iteration t, k_wcol = [Z operators and
// shard sum of A of t, column sums of t-1] beside the W pass of t, whose tiles draw Z; one rank: the
// last chunk also factors Xprec.  Several ranks: k_xred and ONE all-gather of [column sums | A sum |
// X message].  Then k_xdraw = [X operators (several ranks)] beside the X draw, and k_cpass with the
// delta chain of t-1.  Generated draws (Philox, counter-addressed) are drawn where they are consumed
// (Z / X normals, the delta gammas) or in the launch before (k_lambda's normals and gammas: the
// LAMGEN blocks of k_wcol, behind its W tiles).
// The chain of iteration t:  k_wcol -> [k_xred, all-gather] -> k_xdraw -> k_cpass (+ delta of t - 1) ->
// k_lambda, which on a saved iteration also writes the sample into the open assembly batch (loading_rows);
// save_sample then only counts it, launches the probes and hands a full batch to the assembly stream.
struct FusedSchedule {
    dcfm_handle *h;
    const Dims &d;
    const Bufs &b;
    hipStream_t s;                // the main stream
    bool delta_pending = false;   // k_lambda of it - 1 ran, its delta chain not yet queued
    const DrawsDev &draws() const { return d.inject ? h->dr : h->gen[0]; }

    int step(int64_t it) {
        const DrawsDev &dr = draws();
        const bool lamgen = !d.inject;   // k_wcol draws k_lambda's variates (b.ldraw)
        // k_wcol: W pass + the Z draw of the W tiles' rows
        { KTimer t(h, DCFM_K_WPASS, s); launch_wcol(d, b, dr, it, true, delta_pending, true, ++h->wc_ops, s, lamgen); }
        if (d.coll) {   // several ranks: k_xred (the local X message), then ONE all-gather of [column sums
                        // of it - 1 | local A sum | X message]
            { KTimer t(h, DCFM_K_XRED, s); launch_xred(d, b, s); }
            KTimer t(h, DCFM_K_COMM, s);
            TRY(coll_allgather(h, CH_MAIN, b.sloc, b.msg_all, (size_t)d.xstride, s));
        }
        {
            KTimer t(h, DCFM_K_XDRAW, s);
            if (d.coll) launch_xdraw_mr(d, b, dr, it, ++h->xm_ops, s);   // + the X factorisation
            else launch_xdraw(d, b, dr, it, s, true);                    // one rank: sums the shard messages
        }
        {   // k_cpass + the delta chain of it - 1 (column sums from k_wcol / the gather)
            KTimer t(h, DCFM_K_CPASS, s);
            const DeltaTau dt = delta_tau(h);
            if (delta_pending) launch_cpass(d, b, s, dr, dt.delta_in, dt.tau_in, dt.delta_out, dt.tau_out, it - 1);
            else launch_cpass(d, b, s);
        }
        HIPC(h, hipGetLastError());
        if (delta_pending) iteration_done(h);   // outside the timer: it may launch k_trace_part
        TRY(loading_rows(h, dr, it, lamgen));
        delta_pending = true;     // column sums + delta chain ride in the next iteration's launches
        return DCFM_OK;
    }

    // after the loop: the last iteration's column sums (+ their gather) and delta chain
    int tail(int64_t last_iter) {
        if (!delta_pending) return DCFM_OK;
        KTimer t(h, DCFM_K_DELTA, s);
        launch_wcol(d, b, h->dr, last_iter, false, true, false, 0, s);
        if (d.coll) TRY(coll_allgather(h, CH_MAIN, b.sloc, b.msg_all, (size_t)d.xstride, s));
        const DeltaTau dt = delta_tau(h);
        launch_delta(d, b, draws(), last_iter, dt.delta_in, dt.tau_in, dt.delta_out, dt.tau_out, s);   // gammas drawn in place unless injected
        HIPC(h, hipGetLastError());
        iteration_done(h);
        return DCFM_OK;
    }
};

// Generated draws of the side-stream schedule: k_draws batches [b0, b0 + DB) aligned to this call's
// first iteration, queued on the draw stream into a slot whose previous batch the sweep has
// finished with, the next batch while the sweep consumes the current one.
struct DrawBatches {
    dcfm_handle *h;
    int64_t end_iter;
    int64_t batch0, batch_n = 0;   // the batch the sweep is consuming, in h->gen[slot]
    int slot = -1;
    // the slot holding the batch that starts at b0 (queueing it unless it is there), or -1 with
    // the error in the handle; `busy` is the slot the sweep still reads
    int generate(int64_t b0, int busy) {
        hipStream_t sd = h->sdraw;
        const int64_t nb = std::min<int64_t>(h->DB, end_iter - b0);
        for (int sl = 0; sl < 2; ++sl)
            if (h->gen_first[sl] == b0 && h->gen_n[sl] >= nb) return sl;
        int sl = busy >= 0 ? 1 - busy : (h->gen_first[0] <= h->gen_first[1] ? 0 : 1);
        hipError_t e = hipSuccess;
        if (h->used_pending[sl]) {
            e = hipStreamWaitEvent(sd, h->e_used[sl], 0);
            h->used_pending[sl] = false;
        }
        for (int64_t it = b0; e == hipSuccess && it < b0 + nb; ++it) {
            const size_t o = (size_t)(it - b0);
            DrawsDev v = h->gen[sl];
            const size_t *sz = h->draw_iter_sz;
            v.NZ += o * sz[0]; v.NX += o * sz[1]; v.NL += o * sz[2];
            v.Gpsi += o * sz[3]; v.Gdelta += o * sz[4]; v.Gps += o * sz[5];
            v.first_iter = it; v.n_iter = 1;
            KTimer t(h, DCFM_K_DRAWS, sd);
            launch_draws(h->d, v, it, sd);
        }
        if (e == hipSuccess) e = hipEventRecord(h->e_drawn[sl], sd);
        if (e != hipSuccess) {
            fail(h, DCFM_ERR_HIP, "draws batch at iteration %lld: %s", (long long)b0, hipGetErrorString(e));
            return -1;
        }
        h->gen[sl].first_iter = b0;
        h->gen_first[sl] = b0;
        h->gen_n[sl] = nb;
        return sl;
    }

    // before iteration it's first consumer: at a batch boundary the main stream waits for the
    // batch that starts there, and the one after it is queued
    int acquire(int64_t it) {
        if (it != batch0 + batch_n) return DCFM_OK;
        batch0 = it;
        batch_n = std::min<int64_t>(h->DB, end_iter - it);
        slot = generate(it, -1);
        if (slot < 0) return DCFM_ERR_HIP;
        HIPC(h, hipStreamWaitEvent(h->stream, h->e_drawn[slot], 0));
        if (it + batch_n < end_iter && generate(it + batch_n, slot) < 0) return DCFM_ERR_HIP;   // next batch
        return DCFM_OK;
    }

    // iteration it's last consumer is queued
    int release(int64_t it) {
        if (it != batch0 + batch_n - 1) return DCFM_OK;
        HIPC(h, hipEventRecord(h->e_used[slot], h->stream));
        h->used_pending[slot] = true;
        return DCFM_OK;
    }
};

// Side-stream schedule (K > 32, or DCFM_FLAG_UNFUSED): prep and the X operators run on the side
// stream beside the W pass; the draws are injected or read from the k_draws batches.
struct SideSchedule {
    dcfm_handle *h;
    const Dims &d;
    const Bufs &b;
    DrawBatches gen;

    int step(int64_t it) {
        hipStream_t s = h->stream, ss = h->side;
        const size_t KW = d.kp;
        if (!d.inject) TRY(gen.acquire(it));
        const DrawsDev &dr = d.inject ? h->dr : h->gen[gen.slot];
        // side stream: A_m, R_m, Rx from this iteration's incoming Lambda, omega (dc:98-100,112-118)
        HIPC(h, hipStreamWaitEvent(ss, h->e_lam, 0));
        { KTimer t(h, DCFM_K_PREP, ss); launch_prep(d, b, ss); }
        HIPC(h, hipEventRecord(h->e_prep, ss));
        { KTimer t(h, DCFM_K_XCHOL, ss); launch_asum(d, b, ss); }
        if (d.coll) {
            KTimer t(h, DCFM_K_COMM, ss);
            TRY(coll_allgather(h, CH_SIDE, b.xa, b.xa_all, KW * KW, ss));
        }
        { KTimer t(h, DCFM_K_XCHOL, ss); launch_xchol(d, b, ss); }
        HIPC(h, hipEventRecord(h->e_xchol, ss));
        // main stream
        { KTimer t(h, DCFM_K_WPASS, s);  launch_wpass(d, b, s); }
        HIPC(h, hipStreamWaitEvent(s, h->e_prep, 0));
        { KTimer t(h, DCFM_K_ZDRAW, s);  launch_zdraw(d, b, dr, it, s); }
        { KTimer t(h, DCFM_K_XRED, s);   launch_xred(d, b, s); }
        if (d.coll) {
            KTimer t(h, DCFM_K_COMM, s);
            TRY(coll_allgather(h, CH_MAIN, b.xin, b.xall, (size_t)d.NP * KW, s));
        }
        HIPC(h, hipStreamWaitEvent(s, h->e_xchol, 0));
        { KTimer t(h, DCFM_K_XDRAW, s); launch_xdraw(d, b, dr, it, s, false); }
        { KTimer t(h, DCFM_K_CPASS, s); launch_cpass(d, b, s); }
        TRY(loading_rows(h, dr, it, false));
        HIPC(h, hipEventRecord(h->e_lam, s));   // Lambda/omega of this iteration are final
        { KTimer t(h, DCFM_K_COLSUM, s); launch_colsum(d, b, s); }
        if (d.coll) {
            KTimer t(h, DCFM_K_COMM, s);
            TRY(coll_allgather(h, CH_MAIN, b.sloc, b.sall, (size_t)d.G * KW, s));
        }
        {
            KTimer t(h, DCFM_K_DELTA, s);
            const DeltaTau dt = delta_tau(h);
            launch_delta(d, b, dr, it, dt.delta_in, dt.tau_in, dt.delta_out, dt.tau_out, s);
        }
        if (!d.inject) TRY(gen.release(it));
        iteration_done(h);
        return DCFM_OK;
    }
};

int dcfm_run(dcfm_handle *h, int64_t first_iter, int64_t n_iter) {
    TRY(check_run_args(h, first_iter, n_iter));
    HIPC(h, hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    const int64_t end_iter = first_iter + n_iter;
    FusedSchedule fused{h, h->d, h->b, s};
    SideSchedule side{h, h->d, h->b, DrawBatches{h, end_iter, first_iter}};
    if (!h->fused) HIPC(h, hipEventRecord(h->e_lam, s));   // Lambda/omega of the previous iteration are final
    for (int64_t it = first_iter; it < end_iter; ++it) {
        TRY(h->fused ? fused.step(it) : side.step(it));
        HIPC(h, hipGetLastError());
        TRY(save_sample(h, it));
    }
    if (h->fused) TRY(fused.tail(end_iter - 1));
    TRY(flush_batch(h));
    launch_finite(h->d, h->b, delta_tau(h).tau_in, h->nan_dev, s);   // sentinel, read at the next sync point
    HIPC(h, hipGetLastError());
    HIPC(h, hipMemcpyAsync(h->nan_host, h->nan_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    if (h->prof) collect_prof(h);
    return DCFM_OK;
}

int dcfm_set_trace(dcfm_handle *h, int64_t capacity) {
    if (!h || capacity < 0) return fail(h, DCFM_ERR_INVALID, "set_trace: bad argument");
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (h->trace) (void)hipFree(h->trace);
    h->trace = nullptr;
    h->trace_cap = h->trace_n = 0;
    if (capacity == 0) return DCFM_OK;
    const size_t nd = trace_scratch_doubles(h->d.G) + (size_t)capacity * h->d.G * 4;
    if (hipMalloc(&h->trace, nd * sizeof(double)) != hipSuccess)
        return fail(h, DCFM_ERR_ALLOC, "set_trace: %lld rows", (long long)capacity);
    HIPC(h, hipMemset(h->trace, 0, trace_scratch_doubles(h->d.G) * sizeof(double)));   // tickets start at 0
    h->trace_cap = capacity;
    return DCFM_OK;
}

int dcfm_get_trace(dcfm_handle *h, double *out, int64_t *count) {
    if (!h || !count) return fail(h, DCFM_ERR_INVALID, "get_trace: null argument");
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    *count = h->trace_n;
    if (out && h->trace_n) {
        const int G = h->d.G;
        std::vector<double> rows((size_t)h->trace_n * G * 4);
        HIPC(h, hipMemcpy(rows.data(), trace_row(h, 0), rows.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t t = 0; t < h->trace_n; ++t)
            for (int q = 0; q < 4; ++q) {
                double acc = 0.0;
                for (int m = 0; m < G; ++m) acc += rows[((size_t)t * G + m) * 4 + q];   // shard order
                out[t * 4 + q] = acc;
            }
    }
    return DCFM_OK;
}

int dcfm_synchronize(dcfm_handle *h) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    HIPC(h, hipSetDevice(h->cfg.device));
    HIPC(h, hipStreamSynchronize(h->stream));
    HIPC(h, hipStreamSynchronize(h->side));
    HIPC(h, hipStreamSynchronize(h->sdraw));
    HIPC(h, hipStreamSynchronize(h->sasm));
    return numeric_status(h);
}

int64_t dcfm_saved_samples(const dcfm_handle *h) { return h ? h->saved : -1; }

int dcfm_set_profiling(dcfm_handle *h, int enable) {
    return dcfm_set_profiling_mask(h, enable ? 0xFFFFFFFFu : 0u);
}

int dcfm_set_profiling_mask(dcfm_handle *h, uint32_t mask) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    collect_prof(h);
    h->prof_mask = mask;
    h->prof_stride = 1;
    std::fill(h->prof_seq, h->prof_seq + DCFM_K_COUNT, (int64_t)0);
    const bool enable = mask != 0;
    h->prof = enable;
    if (enable) {
        std::fill(h->kms, h->kms + DCFM_K_COUNT, 0.0);
        std::fill(h->kcnt, h->kcnt + DCFM_K_COUNT, 0);
    }
    return DCFM_OK;
}

int dcfm_set_profiling_stride(dcfm_handle *h, int32_t stride) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    if (stride < 1) return fail(h, DCFM_ERR_INVALID, "profiling stride %d < 1", (int)stride);
    h->prof_stride = stride;
    std::fill(h->prof_seq, h->prof_seq + DCFM_K_COUNT, (int64_t)0);
    return DCFM_OK;
}

int dcfm_get_kernel_stats(dcfm_handle *h, double ms[DCFM_K_COUNT], int64_t launches[DCFM_K_COUNT]) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    collect_prof(h);
    for (int k = 0; k < DCFM_K_COUNT; ++k) {
        if (ms) ms[k] = h->kms[k];
        if (launches) launches[k] = h->kcnt[k];
    }
    return DCFM_OK;
}

int dcfm_rng_fill(int device, uint64_t seed, int kind, double shape, int32_t site, int32_t shard,
                  int64_t iter, int64_t count, double *out) {
    if (count < 0) return fail(nullptr, DCFM_ERR_INVALID, "rng_fill: bad argument");
    return dcfm_rng_fill_rows(device, seed, kind, shape, site, shard, iter, (count + 31) / 32, 32, count, out);
}

int dcfm_rng_fill_rows(int device, uint64_t seed, int kind, double shape, int32_t site, int32_t shard,
                       int64_t iter, int64_t rows, int32_t width, int64_t count, double *out) {
    if (!out || count < 0 || rows < 0 || width < 1 || width > (1 << 23) || count > rows * (int64_t)width ||
        (kind != 0 && kind != 1) || (kind == 1 && !(shape > 0.0)))
        return fail(nullptr, DCFM_ERR_INVALID, "rng_fill: bad argument");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, DCFM_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    void *q = nullptr;
    e = hipMalloc(&q, std::max<int64_t>(count, 1) * sizeof(double));
    if (e != hipSuccess) return fail(nullptr, DCFM_ERR_ALLOC, "hipMalloc: %s", hipGetErrorString(e));
    launch_rng_fill(seed, kind, shape, site, shard, iter, count, width, static_cast<double *>(q), nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, q, count * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(q);
    if (e != hipSuccess) return fail(nullptr, DCFM_ERR_HIP, "rng_fill: %s", hipGetErrorString(e));
    return DCFM_OK;
}

}  // extern "C"
