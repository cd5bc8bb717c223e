// Phase stamps of k_wcol's blocks for tools/dev/wstamps.py; WSTAMP(s) is a no-op in the product build.
#pragma once
#include <hip/hip_runtime.h>

namespace dcfm {

#ifdef DCFM_WSTAMPS   // dev build: per-block [start, end] (s_memrealtime, 100 MHz) of the last full k_wcol,
                      // and inside the block [2] OPS: A_m out / W tile: pass done, [3] OPS: U out / W tile:
                      // operators arrived, [4] W tile: operators staged, [5] W tile: first 16-row draw done
__device__ unsigned long long g_wstamps[8192][8];
extern "C" int dcfm_debug_wstamps(unsigned long long *out, int nblocks) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wstamps), (size_t)nblocks * 64, 0, hipMemcpyDeviceToHost);
}
#define WSTAMP(s) do { if (threadIdx.x == 0 && blockIdx.x < 8192) g_wstamps[blockIdx.x][s] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define WSTAMP(s) do { } while (0)
#endif

}  // namespace dcfm
