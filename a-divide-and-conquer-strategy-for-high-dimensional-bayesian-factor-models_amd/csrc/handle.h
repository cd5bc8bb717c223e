// The handle behind the C ABI (include/dcfm.h) and what every host file of libdcfm shares:
// error reporting (fail, HIPC / NCCLC), the profiling timers with their event pool, stream
// synchronisation, and the collectives of comm.hip.  Internal, not installed.
#pragma once
#include "../../include/dcfm.h"
#include "dcfm_internal.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace dcfm;

// everything here is internal to libdcfm.so: only include/dcfm.h is exported
#pragma GCC visibility push(hidden)

struct ProfRec { int kid; hipEvent_t a, b; };
struct LoopGroup;  // in-process loopback collectives (comm.hip)

struct dcfm_handle {
    dcfm_config cfg{};
    Dims d{};
    Bufs b{};
    DrawsDev dr{};
    hipStream_t stream = nullptr;     // main: the sweep chain
    hipStream_t side = nullptr;       // k_prep + k_xchol, overlapping k_wpass (unfused paths)
    hipStream_t sdraw = nullptr;      // on-device Philox variates, a batch ahead of the sweep
    hipStream_t sasm = nullptr;       // covariance assembly, overlapping later iterations
    ncclComm_t comm = nullptr, comm_side = nullptr, comm_asm = nullptr;
    bool comm_ok = false;
    std::shared_ptr<LoopGroup> loop;  // loopback collectives instead of RCCL (testing)
    std::vector<int> Tb;              // Sigma tile-row boundaries of all ranks (block-sharded)
    hipEvent_t lp_ready = nullptr, lp_done = nullptr;
    hipEvent_t e_lam = nullptr, e_prep = nullptr, e_xchol = nullptr, e_batch = nullptr,
               e_free[2] = {nullptr, nullptr}, e_drawn[2] = {nullptr, nullptr}, e_used[2] = {nullptr, nullptr};
    bool fused = false;           // K <= 32 fused launch chain (else the side-stream layout), fixed at create
    bool plam_valid = false;      // b.Plam holds the caller's Plam (no iteration run since set_state)
    unsigned long long wc_ops = 0;   // k_wcol launches with the operator roles (hand-off counter epoch)
    unsigned long long xm_ops = 0;   // k_xdraw launches with the X-operator role (several ranks; its counter's epoch)
    bool asm_pending[2] = {false, false};
    int cur = 0;                  // delta/tau buffer in use
    int lb = 0;                   // Lb buffer being filled
    int B = 16;                   // saved samples per flush
    int batch = 0;                // saved samples pending in Lb[lb]
    int64_t saved = 0;
    bool have_data = false, have_state = false;
    int *nan_dev = nullptr;       // k_finite flag (device) and its pinned host mirror
    int *nan_host = nullptr;
    std::string err;
    std::vector<void *> allocs;
    double *draws_mem = nullptr;
    // on-device Philox draws (no INJECT): two slots of DB iterations, the next batch
    // generated on sdraw while the sweep consumes the current one, so the main stream
    // waits on an event once per batch.  A slot is valid for the iterations it was
    // generated for whatever the state (the stream is counter-based).
    DrawsDev gen[2] = {};
    int64_t gen_first[2] = {-1, -1}, gen_n[2] = {0, 0};
    bool used_pending[2] = {false, false};   // e_used[slot] recorded after the slot's last consumer
    int DB = 1;                              // iterations per draws batch
    size_t draw_iter_sz[6] = {};             // per-iteration doubles of NZ, NX, NL, Gpsi, Gdelta, Gps
    // per-iteration chain trace (dcfm_set_trace): [scratch | rows [trace_cap][G][4]] (trace.hip)
    double *trace = nullptr;
    int64_t trace_cap = 0, trace_n = 0;
    // per-sample probe draws (dcfm_set_probes, probes.hip): one allocation, null when off
    double *probe_mem = nullptr;
    Probes probes{};
    int64_t probe_cap = 0, probe_n = 0;
    // per-sample precision draws (dcfm_set_precision_probes, precision.hip): the same, independent of the probes
    double *prec_mem = nullptr;
    Precision prec{};
    int64_t prec_cap = 0, prec_n = 0;
    // pointwise log-likelihood draws (dcfm_set_loglik, loglik.hip): the same, independent of both
    double *ll_mem = nullptr;
    LogLik ll{};
    int64_t ll_cap = 0, ll_n = 0;
    // conditional prediction (dcfm_set_predict, predict.hip): the same, independent of the three
    double *pred_mem = nullptr;
    Predict pred{};
    int64_t pred_cap = 0, pred_n = 0;
    // missing training data (dcfm_set_missing, impute.hip): one allocation, null when off; imp_cap / imp_n the
    // saved samples the accumulators may hold / hold
    void *imp_mem = nullptr;
    Impute imp{};
    int64_t imp_cap = 0, imp_n = 0;
    // posterior mean of the precision matrix (DCFM_FLAG_PRECISION_MEAN, precision_mean.hip): null when off
    PrecMean pm{};
    // posterior mean and second moment of the partial correlations (DCFM_FLAG_PARTIAL_CORR, partial_corr.hip)
    PartialCorr pc{};
    // posterior mean and second moment of the correlation matrix and of the communalities (DCFM_FLAG_CORR, corr.hip)
    Corr cr{};
    // posterior moments of the regression coefficients (DCFM_FLAG_REGRESSION, dcfm_set_regression, regression.hip):
    // one allocation, null when off; reg_n the saved samples the accumulators hold
    void *reg_mem = nullptr;
    Regress rg{};
    int64_t reg_n = 0;
    bool prof = false;
    uint32_t prof_mask = 0;       // kernel ids (bit DCFM_K_*) timed with events
    int prof_stride = 1;          // time one in prof_stride launches of each (dcfm_set_profiling_stride)
    int64_t prof_seq[DCFM_K_COUNT] = {};   // launches seen per kernel id since the mask was set
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> evpool;
    double kms[DCFM_K_COUNT] = {};
    int64_t kcnt[DCFM_K_COUNT] = {};
};

inline std::string g_err;  // errors without a handle

inline int fail(dcfm_handle *h, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_err = buf;
    return code;
}

#define HIPC(h, x)                                                                        \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess)                                                             \
            return fail(h, DCFM_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                              \
    } while (0)

// return a callee's failure code (its message is already in the handle or g_err)
#define TRY(x) do { if (int rc_ = (x)) return rc_; } while (0)

#define NCCLC(h, x)                                                                      \
    do {                                                                                  \
        ncclResult_t r_ = (x);                                                            \
        if (r_ != ncclSuccess)                                                            \
            return fail(h, DCFM_ERR_RCCL, "%s failed: %s", #x, ncclGetErrorString(r_));   \
    } while (0)

// ---------------------------------------------------------------------------
// collectives: RCCL communicator per stream (CH_*), or the in-process loopback group
// ---------------------------------------------------------------------------
enum { CH_MAIN = 0, CH_SIDE = 1, CH_ASM = 2 };

// comm.hip
int coll_allgather(dcfm_handle *h, int ch, const double *send, double *recv, size_t count, hipStream_t s);
int coll_gather(dcfm_handle *h, const double *send, double *recv, const std::vector<long long> &base,
                const std::vector<long long> &cnt, int root, hipStream_t s);
int coll_allreduce_sum(dcfm_handle *h, int ch, double *buf, size_t count, hipStream_t s);
int agree(dcfm_handle *h, int code);

// ---------------------------------------------------------------------------
// profiling helpers
// ---------------------------------------------------------------------------
inline hipEvent_t get_event(dcfm_handle *h) {
    if (!h->evpool.empty()) {
        hipEvent_t e = h->evpool.back();
        h->evpool.pop_back();
        return e;
    }
    // timing only (read after sync_all): no system-scope fence, whose L2 write-back and
    // invalidate per record cost microseconds and slowed the kernel that followed
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return nullptr;
    return e;
}

struct KTimer {
    dcfm_handle *h;
    int kid;
    hipStream_t s;
    hipEvent_t a = nullptr;
    KTimer(dcfm_handle *h_, int k, hipStream_t s_) : h(h_), kid(k), s(s_) {
        if (h->prof && (h->prof_mask >> k & 1u) && h->prof_seq[k]++ % h->prof_stride == 0) {
            a = get_event(h);
            if (a) (void)hipEventRecord(a, s);
        }
    }
    ~KTimer() {
        if (h->prof && a) {
            hipEvent_t b = get_event(h);
            if (b) {
                (void)hipEventRecord(b, s);
                h->recs.push_back({kid, a, b});
            }
        }
    }
};

inline void sync_all(dcfm_handle *h) {
    (void)hipStreamSynchronize(h->stream);
    if (h->side) (void)hipStreamSynchronize(h->side);
    if (h->sdraw) (void)hipStreamSynchronize(h->sdraw);
    if (h->sasm) (void)hipStreamSynchronize(h->sasm);
}

// DCFM_ERR_NUMERIC once the sentinel of a finished dcfm_run has seen a non-finite state
// (call after the streams are synchronised)
inline int numeric_status(dcfm_handle *h) {
    if (h->nan_host && *h->nan_host)
        return fail(h, DCFM_ERR_NUMERIC, "non-finite sampler state (NaN / Inf in Lambda, ps, omega, X or tau) "
                                         "after dcfm_run; set_state / init_state to restart");
    return DCFM_OK;
}

// impute.hip: forget the mask (dcfm_set_data*: it belongs to the data that is being replaced)
void impute_drop(dcfm_handle *h);

// host generator of the seeded Krylov starts (dcfm_sigma_error, dcfm_sigma_eigs)
inline uint64_t splitmix64(uint64_t &x) {
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#pragma GCC visibility pop
