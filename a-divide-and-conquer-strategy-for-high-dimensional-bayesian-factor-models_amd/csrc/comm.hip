// Collectives of libdcfm: an RCCL communicator per stream, or the in-process loopback group
// (several ranks on one device), and the dcfm_comm_* entry points.
#include "handle.h"

// In-process loopback collectives (dcfm_comm_init_loopback): n handles on one device,
// one host thread per rank, the same all-gather / all-reduce semantics as the RCCL
// communicators — so the multi-rank sweep runs and is parity-tested on a single GPU.
// Per collective: every rank posts its send pointer and a "ready" event (barrier), copies
// every other rank's slice in on its own stream after that rank's event, posts a "done"
// event (barrier), waits for every rank's "done" (no send buffer is reused before all
// ranks read it), and a last barrier frees the posting slots for the next collective.
struct LoopGroup {
    int n;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    std::vector<const double *> send;
    std::vector<hipEvent_t> ready, done;
    explicit LoopGroup(int n_) : n(n_), send(n_, nullptr), ready(n_, nullptr), done(n_, nullptr) {}
    bool barrier(std::unique_lock<std::mutex> &lk) {
        const uint64_t my = gen;
        if (++arrived == n) {
            arrived = 0;
            ++gen;
            cv.notify_all();
            return true;
        }
        return cv.wait_for(lk, std::chrono::seconds(120), [&] { return gen != my; });
    }
};

static int loop_allgather(dcfm_handle *h, const double *send, double *recv, size_t count, hipStream_t s) {
    LoopGroup &G = *h->loop;
    const int r = h->d.rank;
    HIPC(h, hipEventRecord(h->lp_ready, s));
    {
        std::unique_lock<std::mutex> lk(G.mu);
        G.send[r] = send;
        G.ready[r] = h->lp_ready;
        if (!G.barrier(lk)) return fail(h, DCFM_ERR_RCCL, "loopback all-gather: ranks did not meet");
    }
    for (int k = 0; k < G.n; ++k) {
        double *dst = recv + (size_t)k * count;
        if (G.send[k] == dst) continue;                      // in place
        if (k != r) HIPC(h, hipStreamWaitEvent(s, G.ready[k], 0));
        HIPC(h, hipMemcpyAsync(dst, G.send[k], count * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    HIPC(h, hipEventRecord(h->lp_done, s));
    {
        std::unique_lock<std::mutex> lk(G.mu);
        G.done[r] = h->lp_done;
        if (!G.barrier(lk)) return fail(h, DCFM_ERR_RCCL, "loopback all-gather: ranks did not meet");
    }
    for (int k = 0; k < G.n; ++k)
        if (k != r) HIPC(h, hipStreamWaitEvent(s, G.done[k], 0));
    {
        std::unique_lock<std::mutex> lk(G.mu);
        if (!G.barrier(lk)) return fail(h, DCFM_ERR_RCCL, "loopback all-gather: ranks did not meet");
    }
    return DCFM_OK;
}

// Gather to one rank: rank k's cnt[k] doubles land at recv + base[k] on root (recv is
// only read on root; root's own part is already in place when send == recv + base[root]).
static int loop_gather(dcfm_handle *h, const double *send, double *recv, const std::vector<long long> &base,
                       const std::vector<long long> &cnt, int root, hipStream_t s) {
    LoopGroup &G = *h->loop;
    const int r = h->d.rank;
    HIPC(h, hipEventRecord(h->lp_ready, s));
    {
        std::unique_lock<std::mutex> lk(G.mu);
        G.send[r] = send;
        G.ready[r] = h->lp_ready;
        if (!G.barrier(lk)) return fail(h, DCFM_ERR_RCCL, "loopback gather: ranks did not meet");
    }
    if (r == root)
        for (int k = 0; k < G.n; ++k) {
            if (cnt[k] == 0 || G.send[k] == recv + base[k]) continue;
            if (k != r) HIPC(h, hipStreamWaitEvent(s, G.ready[k], 0));
            HIPC(h, hipMemcpyAsync(recv + base[k], G.send[k], cnt[k] * sizeof(double), hipMemcpyDeviceToDevice, s));
        }
    HIPC(h, hipEventRecord(h->lp_done, s));
    {
        std::unique_lock<std::mutex> lk(G.mu);
        G.done[r] = h->lp_done;
        if (!G.barrier(lk)) return fail(h, DCFM_ERR_RCCL, "loopback gather: ranks did not meet");
    }
    if (r != root) HIPC(h, hipStreamWaitEvent(s, G.done[root], 0));   // root has read my buffer
    {
        std::unique_lock<std::mutex> lk(G.mu);
        if (!G.barrier(lk)) return fail(h, DCFM_ERR_RCCL, "loopback gather: ranks did not meet");
    }
    return DCFM_OK;
}

// recv = concatenation over ranks of count doubles (send may be recv + rank * count)
int coll_allgather(dcfm_handle *h, int ch, const double *send, double *recv, size_t count, hipStream_t s) {
    if (h->loop) return loop_allgather(h, send, recv, count, s);
    ncclComm_t c = ch == CH_MAIN ? h->comm : (ch == CH_SIDE ? h->comm_side : h->comm_asm);
    NCCLC(h, ncclAllGather(send, recv, count, ncclDouble, c, s));
    return DCFM_OK;
}

// Point-to-point gather of variable-size parts to `root` (no all-reduce of the data): RCCL
// send / recv in one group on the assembly communicator, or the loopback group.
int coll_gather(dcfm_handle *h, const double *send, double *recv, const std::vector<long long> &base,
                       const std::vector<long long> &cnt, int root, hipStream_t s) {
    if (h->loop) return loop_gather(h, send, recv, base, cnt, root, s);
    const int r = h->d.rank;
    NCCLC(h, ncclGroupStart());
    if (r == root) {
        for (int k = 0; k < h->d.nranks; ++k)
            if (k != root && cnt[k] > 0)
                NCCLC(h, ncclRecv(recv + base[k], (size_t)cnt[k], ncclDouble, k, h->comm_asm, s));
    } else if (cnt[r] > 0) {
        NCCLC(h, ncclSend(send, (size_t)cnt[r], ncclDouble, root, h->comm_asm, s));
    }
    NCCLC(h, ncclGroupEnd());
    return DCFM_OK;
}

// buf = sum over ranks of buf (in rank order for the loopback group)
int coll_allreduce_sum(dcfm_handle *h, int ch, double *buf, size_t count, hipStream_t s) {
    if (!h->loop) {
        ncclComm_t c = ch == CH_MAIN ? h->comm : (ch == CH_SIDE ? h->comm_side : h->comm_asm);
        NCCLC(h, ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, c, s));
        return DCFM_OK;
    }
    void *q = nullptr;
    HIPC(h, hipMalloc(&q, (size_t)h->loop->n * count * sizeof(double)));
    double *all = static_cast<double *>(q);
    int rc = loop_allgather(h, buf, all, count, s);
    if (rc == DCFM_OK) {
        launch_sum_slices(all, h->loop->n, count, buf, s);
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = fail(h, DCFM_ERR_HIP, "loopback all-reduce: %s", hipGetErrorString(e));
    }
    (void)hipFree(all);
    return rc;
}

// Collective entry points (get_sigma_cols, sigma_error) must take the same path on every rank:
// a failure only some ranks see (an argument only the root checks, a non-finite local shard)
// would otherwise leave the others blocked in the collective.  Every rank contributes
// [invalid, numeric, other] failure counts to an all-reduce first; any failure anywhere
// fails the call on all ranks (a rank that saw none reports which failure another rank had).
int agree(dcfm_handle *h, int code) {
    if (!h->d.coll) return code;
    const double f[3] = {code == DCFM_ERR_INVALID ? 1.0 : 0.0, code == DCFM_ERR_NUMERIC ? 1.0 : 0.0,
                         (code != DCFM_OK && code != DCFM_ERR_INVALID && code != DCFM_ERR_NUMERIC) ? 1.0 : 0.0};
    double g[3] = {0.0, 0.0, 0.0};
    const std::string mine = h->err;
    hipError_t e = hipMemcpyAsync(h->b.agree, f, sizeof f, hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess) return fail(h, DCFM_ERR_HIP, "agree: %s", hipGetErrorString(e));
    if (int rc = coll_allreduce_sum(h, CH_ASM, h->b.agree, 3, h->stream)) return rc;
    HIPC(h, hipMemcpyAsync(g, h->b.agree, sizeof g, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (code != DCFM_OK) {
        h->err = mine;
        return code;
    }
    if (g[0] > 0.0) return fail(h, DCFM_ERR_INVALID, "another rank rejected the collective call's arguments");
    if (g[1] > 0.0) return fail(h, DCFM_ERR_NUMERIC, "another rank's sampler state is non-finite");
    if (g[2] > 0.0) return fail(h, DCFM_ERR_HIP, "the collective call failed on another rank");
    return DCFM_OK;
}

extern "C" {

int dcfm_comm_unique_id(uint8_t out[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, DCFM_ERR_RCCL, "ncclGetUniqueId: %s", ncclGetErrorString(r));
    std::memcpy(out, &id, 128);
    return DCFM_OK;
}

int dcfm_comm_init(dcfm_handle *h, const uint8_t id[128]) {
    if (!h || !id) return fail(h, DCFM_ERR_INVALID, "null argument");
    if (!h->d.coll) return DCFM_OK;
    HIPC(h, hipSetDevice(h->cfg.device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    NCCLC(h, ncclCommInitRank(&h->comm, h->d.nranks, uid, h->d.rank));
    // one communicator per stream so collectives on different streams never interleave
    NCCLC(h, ncclCommSplit(h->comm, 0, h->d.rank, &h->comm_side, nullptr));
    NCCLC(h, ncclCommSplit(h->comm, 0, h->d.rank, &h->comm_asm, nullptr));
    h->comm_ok = true;
    return DCFM_OK;
}

int dcfm_comm_init_loopback(dcfm_handle *const *hs, int32_t n) {
    if (!hs || n < 1) return fail(nullptr, DCFM_ERR_INVALID, "null handles or n < 1");
    for (int r = 0; r < n; ++r) {
        if (!hs[r]) return fail(nullptr, DCFM_ERR_INVALID, "null handle %d", r);
        if (hs[r]->d.nranks != n || hs[r]->d.rank != r)
            return fail(hs[r], DCFM_ERR_INVALID, "handle %d: nranks %d rank %d, expected %d / %d", r,
                        hs[r]->d.nranks, hs[r]->d.rank, n, r);
        if (hs[r]->cfg.device != hs[0]->cfg.device)
            return fail(hs[r], DCFM_ERR_INVALID, "loopback ranks must share one device");
    }
    auto G = std::make_shared<LoopGroup>(n);
    for (int r = 0; r < n; ++r) {
        dcfm_handle *h = hs[r];
        HIPC(h, hipSetDevice(h->cfg.device));
        if (!h->lp_ready) HIPC(h, hipEventCreateWithFlags(&h->lp_ready, hipEventDisableTiming));
        if (!h->lp_done) HIPC(h, hipEventCreateWithFlags(&h->lp_done, hipEventDisableTiming));
        h->loop = G;
        h->comm_ok = true;
    }
    return DCFM_OK;
}

}  // extern "C"
