// Test-only device library: one small __global__ wrapper per device primitive of csrc/linalg.h,
// csrc/tile_linalg.h, csrc/delta.h, csrc/gj.h and csrc/slot_tiles.h, so that tests/test_gpu_kunit_*.py can feed each routine
// inputs of their own choosing (tests/kunit_ref.py) instead of the matrices a chain happens to produce.
// The product headers are included unchanged.  Every wrapper stages its operands the way the product caller
// does, calls the routine and stores what it left; block sizes and LDS layouts are the callers'.  One launch
// runs a whole batch (grid = matrices or cases).  Every LDS region handed to a routine is followed by a band
// of GUARD sentinel doubles; guard[block] is 1 if all of them are intact afterwards, else 0.
//
// extern "C" entries: host arrays in, one launch, host arrays out; the return value is the HIP error code.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "linalg.h"
#include "tile_linalg.h"
#include "delta.h"
#include "gj.h"
#include "slot_tiles.h"

using namespace dcfm;

namespace {

constexpr int GUARD = 8;
__device__ __forceinline__ double sentinel() { return __longlong_as_double(0x7ff8dcf0badc0de5ll); }
__device__ __forceinline__ void guard_fill(double *g) {
    for (int e = threadIdx.x; e < GUARD; e += blockDim.x) g[e] = sentinel();
}
__device__ __forceinline__ int guard_ok(const double *g) {
    int ok = 1;
    for (int e = 0; e < GUARD; ++e) ok &= __double_as_longlong(g[e]) == __double_as_longlong(sentinel());
    return ok;
}

// ---------------------------------------------------------------- scalars
__global__ void k_scalar(const double *x, int n, double *rsq, double *rsqh, double *rcp) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        rsq[e] = rsqrt_f64(x[e]);
        rsqh[e] = rsqrt_f64_h(x[e]);
        rcp[e] = rcp_f64(x[e]);
    }
}

// ---------------------------------------------------------------- lane helpers (one wave)
// rows of out (64 lanes each): 0..63 readlane_d(x, row); 64..95 readsel(x, row - 64, lane >= 32);
// 96..99 quad_bcast<0..3>; 100..103 dpp_d<0xB1, 0x4E, 0x124, 0x128>; 104 xor16_d; 105 xor32_d
constexpr int LANE_ROWS = 106;
__global__ __launch_bounds__(64) void k_lanes(const double *x, double *out) {
    const int l = threadIdx.x;
    const double v = x[l];
    static_for<64>([&](auto S) { out[S * 64 + l] = readlane_d(v, S); });
    static_for<32>([&](auto C) { out[(64 + C) * 64 + l] = readsel(v, C, l >= 32); });
    static_for<4>([&](auto J) { out[(96 + J) * 64 + l] = quad_bcast<decltype(J)::value>(v); });
    out[100 * 64 + l] = dpp_d<0xB1>(v);
    out[101 * 64 + l] = dpp_d<0x4E>(v);
    out[102 * 64 + l] = dpp_d<0x124>(v);
    out[103 * 64 + l] = dpp_d<0x128>(v);
    out[104 * 64 + l] = xor16_d(v);
    out[105 * 64 + l] = xor32_d(v);
}

// ---------------------------------------------------------------- wave sums and scans (one wave per case)
__global__ __launch_bounds__(64) void k_sums(const double *x, const double *y, double *rowsum, double *prod,
                                             double *suffix, double *affA, double *affB) {
    const int l = threadIdx.x, e = blockIdx.x * 64 + l;
    rowsum[e] = rowsum16(x[e]);
    prod[e] = wave_scan_prod(x[e], l);
    suffix[e] = wave_suffix_sum(x[e], l);
    double A = x[e], B = y[e];
    affine_scan(A, B, l);
    affA[e] = A;
    affB[e] = B;
}

// ---------------------------------------------------------------- TreeSum (one thread per case)
__global__ void k_tree(const double *src, const int *ns, const int *strides, const long long *offs, int ncase,
                       double *out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncase) return;
    const double *p = src + offs[c];
    const int n = ns[c];
    const size_t st = (size_t)strides[c];
    out[c] = tree_sum(p, n, st);
    out[ncase + c] = tree_sum_f<double, 4>(n, [&](int k) { return p[(size_t)k * st]; });
    TreeSum<double> ts;
    for (int k = 0; k < n; ++k) ts.push(p[(size_t)k * st]);
    out[2 * ncase + c] = n > 0 ? ts.total() : 0.0;
}

// ---------------------------------------------------------------- xcd_remap (one block per total)
__global__ void k_xcd(const int *totals, const int *offs, int *out) {
    const int total = totals[blockIdx.x];
    for (int b = threadIdx.x; b < total; b += blockDim.x) out[offs[blockIdx.x] + b] = xcd_remap(b, total);
}

// ---------------------------------------------------------------- chol_inv16_p (one wave per matrix)
// S: 16 x 16 row-major per matrix.  The block at (o, o) of a 32 x 32 array with pitch LDP is staged as the
// callers stage it: row-major for <KP + 1, false> (zx_ops.h), column-major for <TLD, true> (a tile of
// tile_linalg.h).  Everything else of the array is NaN.  U: the block at (o, o) of Ub, 16 x 16 row-major.
template <int LDP, bool COLMAJ>
__global__ __launch_bounds__(64) void k_chol16p(const double *S, int o, double *U, int *guard) {
    constexpr int REG = 32 * LDP + 32;          // the block at (16, 16) ends at 31 LDP + 31, also for LDP = 17
    __shared__ double Sm[REG + GUARD], Ub[REG + GUARD], lds_l[32 + GUARD], lds_u[16 + GUARD];
    const int lane = threadIdx.x;
    const double *Sg = S + (size_t)blockIdx.x * 256;
    for (int e = lane; e < REG; e += 64) {
        Sm[e] = __builtin_nan("");
        Ub[e] = sentinel();
    }
    guard_fill(Sm + REG); guard_fill(Ub + REG); guard_fill(lds_l + 32); guard_fill(lds_u + 16);
    __syncthreads();
    for (int e = lane; e < 256; e += 64) {
        const int r = e >> 4, c = e & 15;
        Sm[COLMAJ ? (o + c) * LDP + o + r : (o + r) * LDP + o + c] = Sg[e];
    }
    __syncthreads();
    chol_inv16_p<LDP, COLMAJ>(Sm, o, Ub, lds_l, lds_u, lane);
    __syncthreads();
    for (int e = lane; e < 256; e += 64) {
        const int r = e >> 4, c = e & 15;
        U[(size_t)blockIdx.x * 256 + e] = Ub[COLMAJ ? (o + c) * LDP + o + r : (o + r) * LDP + o + c];
    }
    if (lane == 0)
        guard[blockIdx.x] = guard_ok(Sm + REG) & guard_ok(Ub + REG) & guard_ok(lds_l + 32) & guard_ok(lds_u + 16);
}

// ---------------------------------------------------------------- chol_inv16_blk (one wave per matrix)
// S arrives in the fp64 MFMA C/D layout (lane (c16, q) holds S[q + 4 g][c16] in element g), as the wide
// loading-row kernel holds its diagonal tiles; U is stored from the same layout.  HOOK: the hook issues an
// independent MFMA per block step (hk += a b, a = lane + 1, b = 1 / (lane + 1)), stored to hookout.
template <bool HOOK>
__global__ __launch_bounds__(64) void k_chol16blk(const double *S, double *U, double *hookout) {
    const int lane = threadIdx.x, c16 = lane & 15, q = lane >> 4;
    const double *Sg = S + (size_t)blockIdx.x * 256;
    d4 T;
#pragma unroll
    for (int g = 0; g < 4; ++g) T[g] = Sg[(q + 4 * g) * 16 + c16];
    d4 hk = {0.0, 0.0, 0.0, 0.0};
    const double ha = (double)(lane + 1), hb = 1.0 / (double)(lane + 1);
    d4 R;
    if (HOOK) R = chol_inv16_blk(T, lane, [&](auto) { hk = mfma16x16x4(ha, hb, hk); });
    else R = chol_inv16_blk(T, lane, [](auto) {});
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        U[(size_t)blockIdx.x * 256 + (q + 4 * g) * 16 + c16] = R[g];
        hookout[(size_t)blockIdx.x * 256 + (q + 4 * g) * 16 + c16] = hk[g];
    }
}

// ---------------------------------------------------------------- chol_inv32 + mfma_tile32 (256 threads per matrix)
// as prep_ops (zx_ops.h): wave 0 factors Sm (lower triangle; S is stored whole, so the caller's canary in the
// upper triangle is staged too) into Us, then waves 0..3 form T = Us Us' (mfma_tile32<true>) into Sm's place
// and M = T B (mfma_tile32<false>), B a second 32 x 32 matrix
__global__ __launch_bounds__(256) void k_chol32(const double *S, const double *B, double *U, double *Tout, double *Mout,
                                                int *guard) {
    constexpr int REG = KP * (KP + 1), WREG = TS16 * (KP + 1);
    __shared__ double sS[REG + GUARD], sU[REG + GUARD], sB[REG + GUARD], sW[WREG + GUARD], lds_l[32 + GUARD],
        lds_u[16 + GUARD];
    double (*Sm)[KP + 1] = reinterpret_cast<double (*)[KP + 1]>(sS);
    double (*Us)[KP + 1] = reinterpret_cast<double (*)[KP + 1]>(sU);
    double (*Bm)[KP + 1] = reinterpret_cast<double (*)[KP + 1]>(sB);
    double (*Wk)[KP + 1] = reinterpret_cast<double (*)[KP + 1]>(sW);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const size_t mo = (size_t)blockIdx.x * KP * KP;
    for (int e = t; e < REG; e += 256) {
        sS[e] = __builtin_nan("");
        sB[e] = __builtin_nan("");
        sU[e] = sentinel();
    }
    for (int e = t; e < WREG; e += 256) sW[e] = sentinel();
    guard_fill(sS + REG); guard_fill(sU + REG); guard_fill(sB + REG); guard_fill(sW + WREG);
    guard_fill(lds_l + 32); guard_fill(lds_u + 16);
    __syncthreads();
    for (int e = t; e < KP * KP; e += 256) {
        Sm[e / KP][e % KP] = S[mo + e];
        Bm[e / KP][e % KP] = B[mo + e];
    }
    __syncthreads();
    if (wave == 0) chol_inv32(Sm, Us, Wk, lds_l, lds_u, lane);
    __syncthreads();
    const int ti = wave >> 1, tj = wave & 1, j = lane & 15, q = lane >> 4;
    const d4 T = mfma_tile32<true>(Us, Us, ti, tj, lane);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int a = 16 * ti + q + 4 * g, c = 16 * tj + j;
        Sm[a][c] = T[g];
        Tout[mo + a * KP + c] = T[g];
        U[mo + a * KP + c] = Us[a][c];
    }
    __syncthreads();
    const d4 M = mfma_tile32<false>(Sm, Bm, ti, tj, lane);
#pragma unroll
    for (int g = 0; g < 4; ++g) Mout[mo + (16 * ti + q + 4 * g) * KP + 16 * tj + j] = M[g];
    if (t == 0)
        guard[blockIdx.x] = guard_ok(sS + REG) & guard_ok(sU + REG) & guard_ok(sB + REG) & guard_ok(sW + WREG) &
                            guard_ok(lds_l + 32) & guard_ok(lds_u + 16);
}

// ---------------------------------------------------------------- potrf_inv + trtri + uut_store (one block per matrix)
// as k_prep (kernels_wide.hip): S (KW x KW row-major slot per matrix, N x N used) is staged transposed into
// the tiles with the identity pad beyond N.  The guard bands follow the ntiles(nb) tiles the routines own.
constexpr int TILE_KW = 128, TILE_NT = tile::ntiles(TILE_KW / tile::TS);
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_tile(const double *S, const int *Ns, double scale, double *out, double *uout,
                                                  int *guard) {
    __shared__ double Tb[TILE_NT * tile::TSZ + GUARD], Ub[TILE_NT * tile::TSZ + GUARD], lds_l[32 + GUARD],
        lds_u[16 + GUARD];
    const int m = blockIdx.x, N = Ns[m], nb = (N + tile::TS - 1) / tile::TS, t = threadIdx.x;
    const int used = tile::ntiles(nb) * tile::TSZ;
    const double *Am = S + (size_t)m * TILE_KW * TILE_KW;
    for (int e = t; e < used; e += THREADS) {
        Tb[e] = __builtin_nan("");      // the 17th row of a tile's columns is never read
        Ub[e] = sentinel();
    }
    guard_fill(Tb + used); guard_fill(Ub + used); guard_fill(lds_l + 32); guard_fill(lds_u + 16);
    __syncthreads();
    for (int e = t; e < tile::ntiles(nb) * tile::TS * tile::TS; e += THREADS) {
        int I, J;
        tile::tri_pair(e >> 8, I, J);
        const int r = (e >> 4) & 15, c = e & 15, R = 16 * I + r, Cc = 16 * J + c;
        const double v = (R < N && Cc < N) ? Am[(size_t)Cc * TILE_KW + R] : (R == Cc ? 1.0 : 0.0);
        Tb[tile::tix(I, J) * tile::TSZ + c * tile::TLD + r] = v;
    }
    __syncthreads();
    tile::potrf_inv(Tb, Ub, nb, lds_l, lds_u);
    tile::trtri(Tb, Ub, nb);
    double *o = out + (size_t)m * TILE_KW * TILE_KW;
    tile::uut_store(Ub, nb, N, scale, o, TILE_KW, uout + (size_t)m * TILE_KW * TILE_KW);
    __syncthreads();
    if (t == 0) guard[m] = guard_ok(Tb + used) & guard_ok(Ub + used) & guard_ok(lds_l + 32) & guard_ok(lds_u + 16);
}

// ---------------------------------------------------------------- load_shifted + gj_invert + mat_apply (256 threads)
// per matrix m: N = Ns[m], A = I + scale M, Aload = A as loaded, Ainv, logdet, prod = Ainv rhs (N x ncs[m]).
// As in k_precision the global operands have a pitch larger than their extent: M rows GJ_LDM apart, rhs rows
// GJ_LDR, prod rows GJ_LDP (slots of GJ_KW rows); Aload and Ainv are dense N x N in slots of GJ_KW^2.
// Dynamic LDS: A | guard | Cc (16-byte aligned) | guard | sP | guard, sized for GJ_KW.
constexpr int GJ_KW = KP_MAX, GJ_NC = 32, GJ_LDM = GJ_KW + 3, GJ_LDR = GJ_NC + 3, GJ_LDP = GJ_NC + 5;
constexpr size_t gj_lds_doubles() {
    return (size_t)GJ_KW * GJ_KW + GUARD + 1 + (size_t)GJ_KW * GJ_B + GUARD + (size_t)GJ_KW * PREC_PANEL + GUARD;
}
__global__ __launch_bounds__(256) void k_gj(const double *M, const int *Ns, const int *ncs, double scale, const double *rhs,
                                            double *Aload, double *Ainv, double *logdet, double *prod, int *guard) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int m = blockIdx.x, N = Ns[m], nc = ncs[m], t = threadIdx.x;
    double *A = dyn, *gA = A + N * N;
    double *Cc = gA + GUARD + ((N * N) & 1), *gC = Cc + N * GJ_B;
    double *sP = gC + GUARD, *gP = sP + N * PREC_PANEL;
    const size_t mo = (size_t)m * GJ_KW * GJ_KW;
    for (int e = t; e < N * N; e += 256) A[e] = sentinel();
    for (int e = t; e < N * GJ_B; e += 256) Cc[e] = sentinel();
    for (int e = t; e < N * PREC_PANEL; e += 256) sP[e] = sentinel();
    guard_fill(gA); guard_fill(gC); guard_fill(gP);
    __syncthreads();
    load_shifted(A, N, M + (size_t)m * GJ_KW * GJ_LDM, GJ_LDM, scale);
    __syncthreads();
    for (int e = t; e < N * N; e += 256) Aload[mo + e] = A[e];
    const double lg = gj_invert(A, N, Cc);
    for (int e = t; e < N * N; e += 256) Ainv[mo + e] = A[e];
    if (t == 0) logdet[m] = lg;
    mat_apply(A, N, rhs + (size_t)m * GJ_KW * GJ_LDR, GJ_LDR, nc, prod + (size_t)m * GJ_KW * GJ_LDP, GJ_LDP, sP);
    __syncthreads();
    if (t == 0) guard[m] = guard_ok(gA) & guard_ok(gC) & guard_ok(gP);
}

// ---------------------------------------------------------------- suffix_sum_nv + delta_chain (one wave per case)
// as delta_shard: index idx = l + 64 s < K reads t_idx = tau_idx s_idx, G, 1 / delta_old, 1 / delta_ref from
// row `case` of 64 NV doubles; idle indices take the caller's neutral values
template <int NV>
__global__ __launch_bounds__(64) void k_delta(const double *tt, const double *Gm, const double *idold,
                                              const double *idref, const int *Ks, double bd1, double bd2, double *dnew) {
    const int l = threadIdx.x;
    Dims d{};
    d.K = Ks[blockIdx.x];
    d.bd1 = bd1;
    d.bd2 = bd2;
    const size_t ro = (size_t)blockIdx.x * 64 * NV;
    double T[NV], G[NV], io[NV], ir[NV], dn[NV];
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        const int idx = l + 64 * s;
        const bool act = idx < d.K;
        T[s] = act ? tt[ro + idx] : 0.0;
        G[s] = act ? Gm[ro + idx] : 1.0;
        io[s] = act ? idold[ro + idx] : 1.0;
        ir[s] = act ? idref[ro + idx] : 1.0;
    }
    suffix_sum_nv<NV>(T, l);
    delta_chain<NV>(d, l, T, G, io, ir, dn);
#pragma unroll
    for (int s = 0; s < NV; ++s) dnew[ro + l + 64 * s] = dn[s];
}

// ---------------------------------------------------------------- slot_tiles.h
// The per-slot tile loop with the plainest hooks: two row-major panels A, Bm [p][2 KH] (slot s of phase ph at
// columns ph KH + s K), phase 1 staging only the rows of shard sig, a fold that squares the product.  The grid is
// ncase x ntile blocks over the tile list repeated per case; case e / ntile runs ns[case] slots into its own
// tile-packed output
__global__ __launch_bounds__(slot::THREADS) void k_slot(Dims d, const double *__restrict__ A,
                                                        const double *__restrict__ Bm, int KH,
                                                        const int *__restrict__ ns, int ntile, int nph, int sig,
                                                        double inv_eff, const int2 *__restrict__ tiles,
                                                        double *__restrict__ out) {
    __shared__ slot::Panel As, Bs;
    const slot::Tile g(d, tiles, 0);
    const slot::Rows R(g, d);
    const int cs = xcd_remap(blockIdx.x, gridDim.x) / ntile, K = d.K;
    const double *prow[4];
    R.pointers(prow, A, Bm, 2 * (size_t)KH);
    double rg[8];
    auto gload = [&](int s, int ph, int c) {
        const size_t col = (size_t)ph * KH + (size_t)s * K + slot::KC * c;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = R.has(i, c, K) && (ph == 0 || R.shard[i >> 1] == sig);
            rg[i] = ok ? prow[i >> 1][col + 8 * (i & 1)] : 0.0;
        }
    };
    auto lstore = [&](int buf, int) {
#pragma unroll
        for (int i = 0; i < 8; ++i) (i < 4 ? As : Bs)[buf][R.k(i)][R.row(i)] = rg[i];
    };
    d4 acc2[2][4];
    slot::zero(acc2);
    auto fold = [&](int, const d4 (&acc)[2][4]) {
        slot::each([&](int u, int v, int e) { acc2[u][v][e] = fma(acc[u][v][e], acc[u][v][e], acc2[u][v][e]); });
    };
    auto none = [](int, int, int) {};
    if (nph == 1) slot::loop<1>(g, As, Bs, K, ns[cs], 1, gload, lstore, none, none, fold);
    else slot::loop<0>(g, As, Bs, K, ns[cs], nph, gload, lstore, none, none, fold);
    slot::add_tile(g, out + (size_t)cs * ntile * ASM_TILE * ASM_TILE + g.off, d.p, inv_eff, acc2);
}

// ---------------------------------------------------------------- host side
struct Dev {
    void *p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    template <class T> T *as() { return static_cast<T *>(p); }
};
#define KU(x)                              \
    do {                                   \
        const hipError_t e_ = (x);         \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)
int up(Dev &d, const void *h, size_t bytes) {
    KU(hipMalloc(&d.p, bytes ? bytes : 8));
    if (h && bytes) KU(hipMemcpy(d.p, h, bytes, hipMemcpyHostToDevice));
    return 0;
}
int down(void *h, const Dev &d, size_t bytes) {
    if (bytes) KU(hipMemcpy(h, d.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}
int finish() {
    KU(hipGetLastError());
    KU(hipDeviceSynchronize());
    return 0;
}
#define KI(x)                   \
    do {                        \
        const int e_ = (x);     \
        if (e_ != 0) return e_; \
    } while (0)

}  // namespace

extern "C" {

int kunit_scalar(const double *x, int n, double *rsq, double *rsqh, double *rcp) {
    if (n <= 0) return (int)hipErrorInvalidValue;
    const size_t nb = (size_t)n * 8;
    Dev dx, d0, d1, d2_;
    KI(up(dx, x, nb)); KI(up(d0, nullptr, nb)); KI(up(d1, nullptr, nb)); KI(up(d2_, nullptr, nb));
    hipLaunchKernelGGL(k_scalar, dim3(64), dim3(256), 0, 0, dx.as<double>(), n, d0.as<double>(), d1.as<double>(),
                       d2_.as<double>());
    KI(finish());
    KI(down(rsq, d0, nb)); KI(down(rsqh, d1, nb)); KI(down(rcp, d2_, nb));
    return 0;
}

int kunit_lane_rows() { return LANE_ROWS; }
int kunit_lanes(const double *x, double *out) {
    Dev dx, dout;
    KI(up(dx, x, 64 * 8)); KI(up(dout, nullptr, (size_t)LANE_ROWS * 64 * 8));
    hipLaunchKernelGGL(k_lanes, dim3(1), dim3(64), 0, 0, dx.as<double>(), dout.as<double>());
    KI(finish());
    return down(out, dout, (size_t)LANE_ROWS * 64 * 8);
}

int kunit_sums(const double *x, const double *y, int ncase, double *rowsum, double *prod, double *suffix, double *affA,
               double *affB) {
    if (ncase <= 0) return (int)hipErrorInvalidValue;
    const size_t nb = (size_t)ncase * 64 * 8;
    Dev dx, dy, o[5];
    KI(up(dx, x, nb)); KI(up(dy, y, nb));
    for (auto &b : o) KI(up(b, nullptr, nb));
    hipLaunchKernelGGL(k_sums, dim3(ncase), dim3(64), 0, 0, dx.as<double>(), dy.as<double>(), o[0].as<double>(),
                       o[1].as<double>(), o[2].as<double>(), o[3].as<double>(), o[4].as<double>());
    KI(finish());
    KI(down(rowsum, o[0], nb)); KI(down(prod, o[1], nb)); KI(down(suffix, o[2], nb));
    KI(down(affA, o[3], nb)); KI(down(affB, o[4], nb));
    return 0;
}

// case c sums ns[c] values src[offs[c] + k strides[c]]; nsrc = doubles in src (every index is checked against
// it here).  out: [3][ncase] = tree_sum, tree_sum_f<double, 4>, TreeSum::push / total
int kunit_tree(const double *src, long long nsrc, const int *ns, const int *strides, const long long *offs, int ncase,
               double *out) {
    if (ncase <= 0) return (int)hipErrorInvalidValue;
    for (int c = 0; c < ncase; ++c)
        if (ns[c] < 1 || ns[c] >= (1 << TREE_LEVELS) || strides[c] < 1 || offs[c] < 0 ||
            offs[c] + (long long)(ns[c] - 1) * strides[c] >= nsrc)
            return (int)hipErrorInvalidValue;
    Dev ds, dn, dst, dof, dout;
    KI(up(ds, src, (size_t)nsrc * 8)); KI(up(dn, ns, (size_t)ncase * 4)); KI(up(dst, strides, (size_t)ncase * 4));
    KI(up(dof, offs, (size_t)ncase * 8)); KI(up(dout, nullptr, (size_t)3 * ncase * 8));
    hipLaunchKernelGGL(k_tree, dim3((ncase + 63) / 64), dim3(64), 0, 0, ds.as<double>(), dn.as<int>(), dst.as<int>(),
                       dof.as<long long>(), ncase, dout.as<double>());
    KI(finish());
    return down(out, dout, (size_t)3 * ncase * 8);
}

// out: the cases' remaps back to back (case c at the sum of the totals before it)
int kunit_xcd(const int *totals, int ncase, int *out) {
    if (ncase <= 0) return (int)hipErrorInvalidValue;
    int *offs = new int[ncase];
    long long sum = 0;
    for (int c = 0; c < ncase; ++c) {
        if (totals[c] < 1) { delete[] offs; return (int)hipErrorInvalidValue; }
        offs[c] = (int)sum;
        sum += totals[c];
    }
    Dev dt, dof, dout;
    int rc = up(dt, totals, (size_t)ncase * 4);
    if (!rc) rc = up(dof, offs, (size_t)ncase * 4);
    delete[] offs;
    KI(rc);
    KI(up(dout, nullptr, (size_t)sum * 4));
    KU(hipMemset(dout.p, 0xff, (size_t)sum * 4));
    hipLaunchKernelGGL(k_xcd, dim3(ncase), dim3(256), 0, 0, dt.as<int>(), dof.as<int>(), dout.as<int>());
    KI(finish());
    return down(out, dout, (size_t)sum * 4);
}

// variant 0: chol_inv16_p<KP + 1, false>; 1: chol_inv16_p<TLD, true>.  o: 0 or 16
int kunit_chol16p(const double *S, int nmat, int variant, int o, double *U, int *guard) {
    if (nmat <= 0 || (o != 0 && o != 16) || (variant != 0 && variant != 1)) return (int)hipErrorInvalidValue;
    const size_t nb = (size_t)nmat * 256 * 8;
    Dev ds, du, dg;
    KI(up(ds, S, nb)); KI(up(du, nullptr, nb)); KI(up(dg, nullptr, (size_t)nmat * 4));
    KU(hipMemset(dg.p, 0, (size_t)nmat * 4));
    if (variant == 0)
        hipLaunchKernelGGL((k_chol16p<KP + 1, false>), dim3(nmat), dim3(64), 0, 0, ds.as<double>(), o, du.as<double>(),
                           dg.as<int>());
    else
        hipLaunchKernelGGL((k_chol16p<tile::TLD, true>), dim3(nmat), dim3(64), 0, 0, ds.as<double>(), o, du.as<double>(),
                           dg.as<int>());
    KI(finish());
    KI(down(U, du, nb));
    return down(guard, dg, (size_t)nmat * 4);
}

int kunit_chol16blk(const double *S, int nmat, int hook, double *U, double *hookout) {
    if (nmat <= 0) return (int)hipErrorInvalidValue;
    const size_t nb = (size_t)nmat * 256 * 8;
    Dev ds, du, dh;
    KI(up(ds, S, nb)); KI(up(du, nullptr, nb)); KI(up(dh, nullptr, nb));
    if (hook)
        hipLaunchKernelGGL(k_chol16blk<true>, dim3(nmat), dim3(64), 0, 0, ds.as<double>(), du.as<double>(), dh.as<double>());
    else
        hipLaunchKernelGGL(k_chol16blk<false>, dim3(nmat), dim3(64), 0, 0, ds.as<double>(), du.as<double>(), dh.as<double>());
    KI(finish());
    KI(down(U, du, nb));
    return down(hookout, dh, nb);
}

int kunit_chol32(const double *S, const double *B, int nmat, double *U, double *T, double *M, int *guard) {
    if (nmat <= 0) return (int)hipErrorInvalidValue;
    const size_t nb = (size_t)nmat * KP * KP * 8;
    Dev ds, db, du, dt, dm, dg;
    KI(up(ds, S, nb)); KI(up(db, B, nb)); KI(up(du, nullptr, nb)); KI(up(dt, nullptr, nb)); KI(up(dm, nullptr, nb));
    KI(up(dg, nullptr, (size_t)nmat * 4));
    KU(hipMemset(dg.p, 0, (size_t)nmat * 4));
    hipLaunchKernelGGL(k_chol32, dim3(nmat), dim3(256), 0, 0, ds.as<double>(), db.as<double>(), du.as<double>(),
                       dt.as<double>(), dm.as<double>(), dg.as<int>());
    KI(finish());
    KI(down(U, du, nb)); KI(down(T, dt, nb)); KI(down(M, dm, nb));
    return down(guard, dg, (size_t)nmat * 4);
}

// S, out, uout: nmat slots of 128 x 128 doubles (row-major, ld 128); out and uout go up as given, so what
// the routines leave untouched comes back unchanged.  threads: 1024 or 128
int kunit_tile(const double *S, const int *Ns, int nmat, int threads, double scale, double *out, double *uout, int *guard) {
    if (nmat <= 0 || (threads != 1024 && threads != 128)) return (int)hipErrorInvalidValue;
    for (int m = 0; m < nmat; ++m)
        if (Ns[m] < 1 || Ns[m] > TILE_KW) return (int)hipErrorInvalidValue;
    const size_t nb = (size_t)nmat * TILE_KW * TILE_KW * 8;
    Dev ds, dn, dout, du, dg;
    KI(up(ds, S, nb)); KI(up(dn, Ns, (size_t)nmat * 4)); KI(up(dout, out, nb)); KI(up(du, uout, nb));
    KI(up(dg, nullptr, (size_t)nmat * 4));
    KU(hipMemset(dg.p, 0, (size_t)nmat * 4));
    if (threads == 1024)
        hipLaunchKernelGGL(k_tile<1024>, dim3(nmat), dim3(1024), 0, 0, ds.as<double>(), dn.as<int>(), scale,
                           dout.as<double>(), du.as<double>(), dg.as<int>());
    else
        hipLaunchKernelGGL(k_tile<128>, dim3(nmat), dim3(128), 0, 0, ds.as<double>(), dn.as<int>(), scale,
                           dout.as<double>(), du.as<double>(), dg.as<int>());
    KI(finish());
    KI(down(out, dout, nb)); KI(down(uout, du, nb));
    return down(guard, dg, (size_t)nmat * 4);
}

// M: nmat slots of 128 rows of pitch 131 holding an Ns[m] x Ns[m] matrix; Aload, Ainv: slots of 128 x 128
// holding it dense at the start; rhs, prod: slots of 128 rows of pitch 35 and 37 holding Ns[m] x ncs[m].
// prod goes up as given, so what mat_apply leaves untouched comes back unchanged
int kunit_gj(const double *M, const int *Ns, const int *ncs, int nmat, double scale, const double *rhs, double *Aload,
             double *Ainv, double *logdet, double *prod, int *guard) {
    if (nmat <= 0) return (int)hipErrorInvalidValue;
    for (int m = 0; m < nmat; ++m)
        if (Ns[m] < 1 || Ns[m] > GJ_KW || ncs[m] < 1 || ncs[m] > GJ_NC) return (int)hipErrorInvalidValue;
    const size_t nb = (size_t)nmat * GJ_KW * GJ_KW * 8, mb = (size_t)nmat * GJ_KW * GJ_LDM * 8,
                 rb = (size_t)nmat * GJ_KW * GJ_LDR * 8, pb = (size_t)nmat * GJ_KW * GJ_LDP * 8;
    Dev dm, dn, dc, dr, dl, di, dd, dp, dg;
    KI(up(dm, M, mb)); KI(up(dn, Ns, (size_t)nmat * 4)); KI(up(dc, ncs, (size_t)nmat * 4)); KI(up(dr, rhs, rb));
    KI(up(dl, nullptr, nb)); KI(up(di, nullptr, nb)); KI(up(dd, nullptr, (size_t)nmat * 8)); KI(up(dp, prod, pb));
    KI(up(dg, nullptr, (size_t)nmat * 4));
    KU(hipMemset(dg.p, 0, (size_t)nmat * 4));
    KU(hipMemset(dl.p, 0, nb));
    KU(hipMemset(di.p, 0, nb));
    const size_t lds = gj_lds_doubles() * 8;
    KU(hipFuncSetAttribute(reinterpret_cast<const void *>(k_gj), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_gj, dim3(nmat), dim3(256), lds, 0, dm.as<double>(), dn.as<int>(), dc.as<int>(), scale,
                       dr.as<double>(), dl.as<double>(), di.as<double>(), dd.as<double>(), dp.as<double>(), dg.as<int>());
    KI(finish());
    KI(down(Aload, dl, nb)); KI(down(Ainv, di, nb)); KI(down(logdet, dd, (size_t)nmat * 8)); KI(down(prod, dp, pb));
    return down(guard, dg, (size_t)nmat * 4);
}

// nv: 1 (64 indices a case) or 2 (128); the arrays hold ncase rows of 64 nv doubles
int kunit_delta(int nv, const double *tt, const double *G, const double *idold, const double *idref, const int *Ks,
                int ncase, double bd1, double bd2, double *dnew) {
    if (ncase <= 0 || (nv != 1 && nv != 2)) return (int)hipErrorInvalidValue;
    for (int c = 0; c < ncase; ++c)
        if (Ks[c] < 1 || Ks[c] > 64 * nv) return (int)hipErrorInvalidValue;
    const size_t nb = (size_t)ncase * 64 * nv * 8;
    Dev d0, d1, d2_, d3, dk, dout;
    KI(up(d0, tt, nb)); KI(up(d1, G, nb)); KI(up(d2_, idold, nb)); KI(up(d3, idref, nb));
    KI(up(dk, Ks, (size_t)ncase * 4)); KI(up(dout, nullptr, nb));
    if (nv == 1)
        hipLaunchKernelGGL(k_delta<1>, dim3(ncase), dim3(64), 0, 0, d0.as<double>(), d1.as<double>(), d2_.as<double>(),
                           d3.as<double>(), dk.as<int>(), bd1, bd2, dout.as<double>());
    else
        hipLaunchKernelGGL(k_delta<2>, dim3(ncase), dim3(64), 0, 0, d0.as<double>(), d1.as<double>(), d2_.as<double>(),
                           d3.as<double>(), dk.as<int>(), bd1, bd2, dout.as<double>());
    KI(finish());
    return down(dnew, dout, nb);
}

// A, B: [p][2 KH] row-major; ns: the cases' slot counts; out: ncase tile-packed lower triangles of
// cdiv(p, 128) tile rows (128 x 128 doubles a tile), which go up as given and come back with the sums added
int kunit_slot(const double *A, const double *B, int p, int P, int K, int KH, const int *ns, int ncase, int nph, int sig,
               double inv_eff, double *out) {
    if (p <= 0 || P <= 0 || p % P || K < 1 || K > KH || ncase <= 0 || (nph != 1 && nph != 2)) return (int)hipErrorInvalidValue;
    for (int c = 0; c < ncase; ++c)
        if (ns[c] < 0 || (long long)ns[c] * K > KH) return (int)hipErrorInvalidValue;   // every slot inside its phase's half
    const int nt = (p + ASM_TILE - 1) / ASM_TILE, ntile = nt * (nt + 1) / 2;
    int2 *tl = new int2[(size_t)ncase * ntile];
    for (int c = 0, e = 0; c < ncase; ++c)
        for (int ti = 0; ti < nt; ++ti)
            for (int tj = 0; tj <= ti; ++tj) tl[e++] = make_int2(ti, tj);
    Dims d{};
    d.p = p, d.P = P, d.g = p / P, d.K = K;
    const size_t pb = (size_t)p * 2 * KH * 8, ob = (size_t)ncase * ntile * ASM_TILE * ASM_TILE * 8;
    Dev da, db, dn, dt, dout;
    int rc = up(dt, tl, (size_t)ncase * ntile * sizeof(int2));
    delete[] tl;
    KI(rc);
    KI(up(da, A, pb)); KI(up(db, B, pb)); KI(up(dn, ns, (size_t)ncase * 4)); KI(up(dout, out, ob));
    hipLaunchKernelGGL(k_slot, dim3(ncase * ntile), dim3(slot::THREADS), 0, 0, d, da.as<double>(), db.as<double>(), KH,
                       dn.as<int>(), ntile, nph, sig, inv_eff, dt.as<int2>(), dout.as<double>());
    KI(finish());
    return down(out, dout, ob);
}

}  // extern "C"
