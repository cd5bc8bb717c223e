// What the host files of the Sigmaout operator share (sigma_eigs.hip: dcfm_sigma_apply, dcfm_sigma_eigs;
// sigma_solve.hip: dcfm_sigma_solve): the device scratch of the apply passes of one call and the
// common entry sequence.  Internal, not installed.
#pragma once
#include "handle.h"

#pragma GCC visibility push(hidden)

constexpr int APPLY_NB = 32;   // right-hand sides per kernel pass

// device scratch of the apply passes of one call: V and Y blocks (p x 32 each) and the kernel's
// partial panels, then `extra` doubles of the caller's own (more); every part starts on a 16-byte
// boundary.  Allocated inside the call and freed before it returns
struct ApplyScratch {
    double *dev = nullptr, *dV = nullptr, *dY = nullptr, *part = nullptr, *more = nullptr;
    hipEvent_t ea = nullptr, eb = nullptr;
    int alloc(dcfm_handle *h, int nv_max, const char *who, size_t extra = 0) {
        const size_t P = (size_t)h->d.p, w = (size_t)std::min(nv_max, APPLY_NB);
        const size_t panel = (P * w + 1) & ~(size_t)1, np = (sigma_apply_scratch(h->b.T0, h->b.T1, (int)w) + 1) & ~(size_t)1;
        const size_t nd = 2 * panel + np + extra;
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(nd, 1) * sizeof(double));
        if (e != hipSuccess) return fail(h, DCFM_ERR_ALLOC, "%s: %zu doubles of scratch: %s", who, nd, hipGetErrorString(e));
        dev = static_cast<double *>(q);
        dV = dev;
        dY = dV + panel;
        part = dY + panel;
        more = part + np;
        ea = get_event(h);
        eb = get_event(h);
        return DCFM_OK;
    }
    void release(dcfm_handle *h) {
        if (dev) (void)hipFree(dev);
        if (ea) h->evpool.push_back(ea);
        if (eb) h->evpool.push_back(eb);
        dev = nullptr;
        ea = eb = nullptr;
    }
};

// arguments are checked, the device selected, the streams drained and the sentinel read, in the
// order of dcfm_sigma_error; `code` carries an earlier argument failure
inline int sigma_op_enter(dcfm_handle *h, int code, const char *who) {
    if (code == DCFM_OK) {
        const hipError_t e = hipSetDevice(h->cfg.device);
        if (e != hipSuccess) code = fail(h, DCFM_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    sync_all(h);
    if (code == DCFM_OK) code = numeric_status(h);
    return code;
}

#pragma GCC visibility pop
