// Hand-off between blocks of one launch (k_wcol's roles, k_xdraw's operator block, k_trace_part's
// slices): the payload goes out by agent-scope stores, the storing threads wait for them
// (s_waitcnt vmcnt(0)) and meet at the workgroup barrier, then one thread bumps a relaxed
// agent-scope counter; a consumer reads the payload with agent-scope loads once the counter says so.
//
// Hardware assumption (not the HIP memory model's release / acquire, which on gfx950 costs an
// L2 write-back + invalidate per hand-off — __threadfence's buffer_wbl2 / buffer_inv flush the
// XCD's whole L2 and drop what co-resident blocks cache: +25 us per k_wcol in round 1, +20 us
// next to a Y pass): this is the guide's cross-XCD hand-off recipe -- (1) every payload store is
// an agent-scope (sc1) atomic store that bypasses the non-coherent per-XCD L2 copy, (2) the
// storing threads wait for those stores (s_waitcnt vmcnt(0)) and meet at the workgroup barrier
// before one thread signals, (3) the counter is an atomic, (4) every consumer load of the payload
// is an agent-scope (sc1) load issued after the counter was read.  An ISA without sc1 coherence
// for relaxed agent-scope atomics would break it; tests/test_gpu_loopback.py, test_gpu_trace.py
// and the parity tests run these paths.
#pragma once
#include <hip/hip_runtime.h>

namespace dcfm {

// Agent-scope (all XCDs) coherent access to the payload: relaxed atomics bypass the
// non-coherent per-XCD L2 copies (sc1), no L2 flush needed.
__device__ __forceinline__ void st_agent(double *p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_agent(const double *p) {
    return __hip_atomic_load(const_cast<double *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the block's stores are done (every thread calls): its threads have waited for them and met
__device__ __forceinline__ void stores_done() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this thread's agent-scope stores are done
    __syncthreads();
}

// Producer / consumers: a monotonic 64-bit counter, bumped once per producer block; consumers
// poll it (s_sleep) up to the launch's target.
__device__ __forceinline__ void signal_count(unsigned long long *ctr) {
    stores_done();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wait_count(unsigned long long *ctr, unsigned long long target) {
    if (threadIdx.x == 0)
        while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) __builtin_amdgcn_s_sleep(1);
    __syncthreads();
}

// Last arrival: `count` blocks publish their parts and take a ticket; the block that draws the
// last one (true, for all its threads) reads every part and resets the ticket for the next
// launch.  flag: one LDS word, free again on return.
__device__ __forceinline__ bool last_arrival(unsigned *ticket, unsigned count, unsigned *flag) {
    stores_done();
    if (threadIdx.x == 0) {
        const bool last =
            __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == count - 1;
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // next launch
        *flag = last ? 1u : 0u;
    }
    __syncthreads();
    const bool last = *flag != 0u;
    __syncthreads();
    return last;
}

}  // namespace dcfm
