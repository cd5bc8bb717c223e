// X = Sigmaout^{-1} B on the device (dcfm_sigma_solve): conjugate gradients on the apply pass of
// sigma_apply.hip, up to 32 right-hand sides in lock-step.  Every column runs its own CG (its own
// alpha, beta and stop test; no nv x nv coupling), a pass W = Sigmaout P serves all of them, and
// the panels X, R, P, W, B (p x 32 column-major, leading dimension p) stay in HBM from the upload
// of B to the download of X: per iteration the host reads the columns' done flags and nothing else.
//
//   start   X = 0, R = P = B, rr = B.B                                  k_cg_start, k_cg_state0
//   step    W = Sigmaout P  (all-reduced over the ranks)                launch_sigma_apply
//           pw = P.W                                                    k_panel_dot
//           alpha = rr / pw;  X += alpha P;  R -= alpha W;  rr' = R.R   k_cg_xr
//           beta = rr' / rr;  P = R + beta P;  done = |R| <= tol |B|    k_cg_p
//   finish  W = Sigmaout X;  |B - W| / |B|,  B.X                         k_panel_dot, k_cg_finish
//
// Reductions are deterministic and a function of p alone: column c is the grid's y index, its rows
// are walked in pairs by solve_blocks(p) blocks of 256 threads (thread t of block b takes the rows
// 2 (256 b + t) + 512 solve_blocks(p) i, i = 0, 1, ..), a block's sum is the wave butterfly (DPP
// within a row of 16 lanes, permlane swaps across the rows) of lane 0 and the four waves in wave
// order, and the blocks' partials are added in block order.  So neither the other columns of the
// call nor the column's position among them reach its bits.  The scalars of a step are formed from
// the partials by every block that needs them (at most 64 uniform loads), which saves a one-block
// launch between the sweeps; the column's state is double-buffered, read from st and written to
// st_next by block 0 of k_cg_p, so no block reads what another writes in the same launch.
//
// A column is frozen (alpha = beta = 0: X, R, P untouched from then on) once it has stopped, when B_c
// is zero or non-finite, and when P.W is not a positive finite number (Sigmaout is positive
// definite once a sample is saved, so that means rounding has exhausted the column): no NaN from a
// division reaches X.
//
// Traffic per step besides the pass (4 p^2 bytes): 11 panel sweeps, k_panel_dot 2 reads, k_cg_xr
// 4 reads + 2 writes, k_cg_p 2 reads + 1 write: 88 p nv bytes.
#include "sigma_op.h"
#include "linalg.h"

namespace dcfm {

constexpr int SOLVE_T = 256;              // threads of a panel block
constexpr int SOLVE_ROWS = 2 * SOLVE_T;   // rows of a column a block takes per step (a pair per thread)
constexpr int SOLVE_NB = 64;              // most blocks per column; x 32 columns = the 2048-block cap

// state of one column's recurrence
struct CgCol {
    double rr, bb;      // R.R of the current residual, B.B
    int done, iters;    // frozen; CG steps taken
};

inline int solve_blocks(int p) { return std::min(cdiv(p, SOLVE_ROWS), SOLVE_NB); }

// rows (a, a + 1), a even, of a column: one 16-byte access where the column starts on a 16-byte
// boundary (al; every panel does when p is even), else two of 8; rows >= p read as 0 and are not written
__device__ __forceinline__ d2 ld2(const double *__restrict__ col, int a, int p, bool al) {
    d2 v = {0.0, 0.0};
    if (al && a + 1 < p) {
        v = *reinterpret_cast<const d2 *>(col + a);
    } else {
        if (a < p) v.x = col[a];
        if (a + 1 < p) v.y = col[a + 1];
    }
    return v;
}
__device__ __forceinline__ void st2(double *__restrict__ col, int a, int p, bool al, d2 v) {
    if (al && a + 1 < p) {
        *reinterpret_cast<d2 *>(col + a) = v;
    } else {
        if (a < p) col[a] = v.x;
        if (a + 1 < p) col[a + 1] = v.y;
    }
}
__device__ __forceinline__ bool aligned16(const double *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// the sum of v over the block's 256 threads in a fixed order, in every thread: lane 0's butterfly sum of
// each wave (rows of 16 lanes by DPP, then the rows by permlane swaps), the four waves in wave order
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = rowsum16(v);
    v += xor16_d(v);
    v += xor32_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// a column's dot product from its blocks' partials, in block order
__device__ __forceinline__ double sum_partials(const double *__restrict__ part, int nblk) {
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[b];
    return s;
}

// a step moves column c (not frozen, P.W a positive finite number); the same bits in k_cg_xr and k_cg_p
__device__ __forceinline__ bool cg_live(const CgCol &s, double pw) { return !s.done && pw > 0.0 && pw < INFINITY; }

// part[c][block] = this block's share of A_c . B_c (OP 0) or |A_c - B_c|^2 (OP 1) over the rows of
// column c; grid (solve_blocks(p), columns).  The tall-skinny inner product of the operator files
template <int OP>
__global__ __launch_bounds__(SOLVE_T) void k_panel_dot(const double *__restrict__ A, const double *__restrict__ B,
                                                       int p, double *__restrict__ part) {
    __shared__ double red[4];
    const int c = blockIdx.y;
    const double *__restrict__ a_ = A + (size_t)c * p, *__restrict__ b_ = B + (size_t)c * p;
    const bool al = aligned16(a_) && aligned16(b_);
    double acc = 0.0;
    for (int a = 2 * (blockIdx.x * SOLVE_T + threadIdx.x); a < p; a += gridDim.x * SOLVE_ROWS) {
        const d2 x = ld2(a_, a, p, al), y = ld2(b_, a, p, al);
        if (OP == 0) {
            acc = fma(x.x, y.x, acc);
            acc = fma(x.y, y.y, acc);
        } else {
            const double d0 = x.x - y.x, d1 = x.y - y.y;
            acc = fma(d0, d0, acc);
            acc = fma(d1, d1, acc);
        }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) part[c * SOLVE_NB + blockIdx.x] = s;
}

// X = 0, R = P = B and the partials of B.B
__global__ __launch_bounds__(SOLVE_T) void k_cg_start(const double *__restrict__ B, int p, double *__restrict__ X,
                                                      double *__restrict__ R, double *__restrict__ P,
                                                      double *__restrict__ part) {
    __shared__ double red[4];
    const int c = blockIdx.y;
    const size_t o = (size_t)c * p;
    const bool al = aligned16(B + o) && aligned16(X + o) && aligned16(R + o) && aligned16(P + o);
    double acc = 0.0;
    for (int a = 2 * (blockIdx.x * SOLVE_T + threadIdx.x); a < p; a += gridDim.x * SOLVE_ROWS) {
        const d2 b = ld2(B + o, a, p, al);
        st2(X + o, a, p, al, d2{0.0, 0.0});
        st2(R + o, a, p, al, b);
        st2(P + o, a, p, al, b);
        acc = fma(b.x, b.x, acc);
        acc = fma(b.y, b.y, acc);
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) part[c * SOLVE_NB + blockIdx.x] = s;
}

// the columns' first state: rr = bb = B.B; a zero or non-finite column is frozen at X = 0
__global__ void k_cg_state0(const double *__restrict__ part, int nblk, int w, CgCol *__restrict__ st,
                            int *__restrict__ flags) {
    const int c = threadIdx.x;
    if (c >= w) return;
    const double bb = sum_partials(part + c * SOLVE_NB, nblk);
    const int done = !(bb > 0.0 && bb < INFINITY);
    st[c] = CgCol{bb, bb, done, 0};
    flags[c] = done;
}

// alpha = rr / P.W;  X += alpha P;  R -= alpha W;  the partials of the new R.R
__global__ __launch_bounds__(SOLVE_T) void k_cg_xr(const double *__restrict__ P, const double *__restrict__ W, int p,
                                                   const CgCol *__restrict__ st, const double *__restrict__ part_pw,
                                                   int nblk, double *__restrict__ X, double *__restrict__ R,
                                                   double *__restrict__ part_rr) {
    __shared__ double red[4];
    const int c = blockIdx.y;
    const CgCol s = st[c];
    const double pw = sum_partials(part_pw + c * SOLVE_NB, nblk);
    const bool live = cg_live(s, pw);
    const double alpha = live ? s.rr / pw : 0.0;
    if (!live) return;                               // frozen (block-uniform): X, R and the partials stay
    const size_t o = (size_t)c * p;
    const bool al = aligned16(P + o) && aligned16(W + o) && aligned16(X + o) && aligned16(R + o);
    double acc = 0.0;
    for (int a = 2 * (blockIdx.x * SOLVE_T + threadIdx.x); a < p; a += gridDim.x * SOLVE_ROWS) {
        const d2 pp = ld2(P + o, a, p, al), ww = ld2(W + o, a, p, al);
        d2 x = ld2(X + o, a, p, al), r = ld2(R + o, a, p, al);
        x.x = fma(alpha, pp.x, x.x);
        x.y = fma(alpha, pp.y, x.y);
        r.x = fma(-alpha, ww.x, r.x);
        r.y = fma(-alpha, ww.y, r.y);
        st2(X + o, a, p, al, x);
        st2(R + o, a, p, al, r);
        acc = fma(r.x, r.x, acc);
        acc = fma(r.y, r.y, acc);
    }
    const double sum = block_sum(acc, red);
    if (threadIdx.x == 0) part_rr[c * SOLVE_NB + blockIdx.x] = sum;
}

// beta = rr' / rr;  P = R + beta P;  the column's next state (block 0) and its done flag
__global__ __launch_bounds__(SOLVE_T) void k_cg_p(const double *__restrict__ R, int p, const CgCol *__restrict__ st,
                                                  CgCol *__restrict__ st_next, const double *__restrict__ part_pw,
                                                  const double *__restrict__ part_rr, int nblk, double tol,
                                                  double *__restrict__ P, int *__restrict__ flags) {
    const int c = blockIdx.y;
    const CgCol s = st[c];
    const double pw = sum_partials(part_pw + c * SOLVE_NB, nblk);
    const bool live = cg_live(s, pw);
    const double rr = live ? sum_partials(part_rr + c * SOLVE_NB, nblk) : s.rr;
    // stopped, or the residual norm is no number any more; a column that did not move never will
    const bool done = !live || !(rr < INFINITY) || sqrt(rr) <= tol * sqrt(s.bb);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st_next[c] = CgCol{rr, s.bb, done ? 1 : 0, s.iters + (live ? 1 : 0)};
        flags[c] = done ? 1 : 0;
    }
    const double beta = done ? 0.0 : rr / s.rr;
    if (done) return;                                // frozen (block-uniform): P stays
    const size_t o = (size_t)c * p;
    const bool al = aligned16(R + o) && aligned16(P + o);
    for (int a = 2 * (blockIdx.x * SOLVE_T + threadIdx.x); a < p; a += gridDim.x * SOLVE_ROWS) {
        const d2 r = ld2(R + o, a, p, al);
        d2 pp = ld2(P + o, a, p, al);
        pp.x = fma(beta, pp.x, r.x);
        pp.y = fma(beta, pp.y, r.y);
        st2(P + o, a, p, al, pp);
    }
}

// out[0][c] = |B_c - Sigmaout X_c| / |B_c| (0 for a zero column), out[1][c] = B_c . X_c, out[2][c] = steps
__global__ void k_cg_finish(const CgCol *__restrict__ st, const double *__restrict__ part_res,
                            const double *__restrict__ part_bx, int nblk, int w, double *__restrict__ out) {
    const int c = threadIdx.x;
    if (c >= w) return;
    const CgCol s = st[c];
    const double res = sum_partials(part_res + c * SOLVE_NB, nblk);
    out[c] = s.bb == 0.0 ? 0.0 : sqrt(res) / sqrt(s.bb);
    out[APPLY_NB + c] = sum_partials(part_bx + c * SOLVE_NB, nblk);
    out[2 * APPLY_NB + c] = (double)s.iters;
}

}  // namespace dcfm

#pragma GCC visibility push(hidden)
namespace {

// the call's own device memory behind ApplyScratch's (dV = P, dY = W): the panels B, X, R, the
// partials of four dot products, the result rows, the two states and the flags
struct SolveMem {
    double *B, *X, *R, *ppw, *prr, *pres, *pbx, *out;
    CgCol *st;
    int *flags;
    static size_t panel(size_t P, int w) { return (P * w + 1) & ~(size_t)1; }
    static size_t doubles(size_t P, int w) {
        return 3 * panel(P, w) + 4 * APPLY_NB * SOLVE_NB + 3 * APPLY_NB + 2 * APPLY_NB * sizeof(CgCol) / sizeof(double) +
               APPLY_NB * sizeof(int) / sizeof(double);
    }
    SolveMem(double *q, size_t P, int w) {
        B = q;
        X = B + panel(P, w);
        R = X + panel(P, w);
        ppw = R + panel(P, w);
        prr = ppw + APPLY_NB * SOLVE_NB;
        pres = prr + APPLY_NB * SOLVE_NB;
        pbx = pres + APPLY_NB * SOLVE_NB;
        out = pbx + APPLY_NB * SOLVE_NB;
        st = reinterpret_cast<CgCol *>(out + 3 * APPLY_NB);
        flags = reinterpret_cast<int *>(st + 2 * APPLY_NB);
    }
};
static_assert(sizeof(CgCol) % sizeof(double) == 0, "the states are carved out of a double array");

struct SolveEvents {
    hipEvent_t a[4] = {nullptr, nullptr, nullptr, nullptr};   // around the pass, around the panel kernels
    void get(dcfm_handle *h) { for (auto &e : a) e = get_event(h); }
    void release(dcfm_handle *h) {
        for (auto &e : a) {
            if (e) h->evpool.push_back(e);
            e = nullptr;
        }
    }
    bool all() const { return a[0] && a[1] && a[2] && a[3]; }
};

// the columns [c0, c0 + w) of the solve, w <= 32
int solve_chunk(dcfm_handle *h, ApplyScratch &sc, SolveMem &m, SolveEvents &ev, const double *B, int w, double tol,
                int max_iter, double *X, double *relres, int32_t *iters, double *quad, double *ms) {
    const int p = h->d.p, nblk = solve_blocks(p);
    const size_t bytes = (size_t)p * w * sizeof(double);
    const dim3 grid(nblk, w), blk(SOLVE_T);
    hipStream_t s = h->stream;
    double *dP = sc.dV, *dW = sc.dY;
    const bool timed = ms && ev.all();
    int flags[APPLY_NB];
    HIPC(h, hipMemcpyAsync(m.B, B, bytes, hipMemcpyHostToDevice, s));
    if (timed) HIPC(h, hipEventRecord(ev.a[2], s));
    hipLaunchKernelGGL(k_cg_start, grid, blk, 0, s, m.B, p, m.X, m.R, dP, m.prr);
    hipLaunchKernelGGL(k_cg_state0, dim3(1), dim3(64), 0, s, m.prr, nblk, w, m.st, m.flags);
    HIPC(h, hipGetLastError());
    if (timed) {
        HIPC(h, hipEventRecord(ev.a[3], s));
        HIPC(h, hipStreamSynchronize(s));
        float t = 0.f;
        HIPC(h, hipEventElapsedTime(&t, ev.a[2], ev.a[3]));
        *ms += t;
    }
    int g = 0;
    for (int it = 0; it < max_iter; ++it) {
        if (timed) HIPC(h, hipEventRecord(ev.a[0], s));
        launch_sigma_apply(h->b.Sigma, p, h->b.T0, h->b.T1, dP, w, sc.part, dW, s);
        HIPC(h, hipGetLastError());
        if (timed) HIPC(h, hipEventRecord(ev.a[1], s));
        if (h->d.coll) TRY(coll_allreduce_sum(h, CH_ASM, dW, (size_t)p * w, s));
        if (timed) HIPC(h, hipEventRecord(ev.a[2], s));
        hipLaunchKernelGGL(k_panel_dot<0>, grid, blk, 0, s, dP, dW, p, m.ppw);
        hipLaunchKernelGGL(k_cg_xr, grid, blk, 0, s, dP, dW, p, m.st + g * APPLY_NB, m.ppw, nblk, m.X, m.R, m.prr);
        hipLaunchKernelGGL(k_cg_p, grid, blk, 0, s, m.R, p, m.st + g * APPLY_NB, m.st + (g ^ 1) * APPLY_NB, m.ppw, m.prr,
                           nblk, tol, dP, m.flags);
        HIPC(h, hipGetLastError());
        g ^= 1;
        if (timed) HIPC(h, hipEventRecord(ev.a[3], s));
        HIPC(h, hipMemcpyAsync(flags, m.flags, w * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPC(h, hipStreamSynchronize(s));
        if (timed) {
            float t0 = 0.f, t1 = 0.f;
            HIPC(h, hipEventElapsedTime(&t0, ev.a[0], ev.a[1]));
            HIPC(h, hipEventElapsedTime(&t1, ev.a[2], ev.a[3]));
            *ms += t0 + t1;
        }
        bool all = true;
        for (int c = 0; c < w; ++c) all = all && flags[c] != 0;
        if (all) break;
    }
    // the residual of the returned X from a real pass, and B.X
    if (timed) HIPC(h, hipEventRecord(ev.a[0], s));
    launch_sigma_apply(h->b.Sigma, p, h->b.T0, h->b.T1, m.X, w, sc.part, dW, s);
    HIPC(h, hipGetLastError());
    if (timed) HIPC(h, hipEventRecord(ev.a[1], s));
    if (h->d.coll) TRY(coll_allreduce_sum(h, CH_ASM, dW, (size_t)p * w, s));
    if (timed) HIPC(h, hipEventRecord(ev.a[2], s));
    hipLaunchKernelGGL(k_panel_dot<1>, grid, blk, 0, s, m.B, dW, p, m.pres);
    hipLaunchKernelGGL(k_panel_dot<0>, grid, blk, 0, s, m.B, m.X, p, m.pbx);
    hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(64), 0, s, m.st + g * APPLY_NB, m.pres, m.pbx, nblk, w, m.out);
    HIPC(h, hipGetLastError());
    if (timed) HIPC(h, hipEventRecord(ev.a[3], s));
    double out[3 * APPLY_NB];
    HIPC(h, hipMemcpyAsync(X, m.X, bytes, hipMemcpyDeviceToHost, s));
    HIPC(h, hipMemcpyAsync(out, m.out, sizeof out, hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));
    if (timed) {
        float t0 = 0.f, t1 = 0.f;
        HIPC(h, hipEventElapsedTime(&t0, ev.a[0], ev.a[1]));
        HIPC(h, hipEventElapsedTime(&t1, ev.a[2], ev.a[3]));
        *ms += t0 + t1;
    }
    for (int c = 0; c < w; ++c) {
        relres[c] = out[c];
        if (quad) quad[c] = out[APPLY_NB + c];
        if (iters) iters[c] = (int32_t)out[2 * APPLY_NB + c];
    }
    return DCFM_OK;
}

}  // namespace
#pragma GCC visibility pop

extern "C" int dcfm_sigma_solve(dcfm_handle *h, const double *B, int32_t nv, double tol, int32_t max_iter, double *X,
                                double *relres, int32_t *iters, double *quad, double *dev_ms) {
    if (!h) return fail(h, DCFM_ERR_INVALID, "null handle");
    int code = DCFM_OK;
    if (!B || !X || !relres) code = fail(h, DCFM_ERR_INVALID, "null argument");
    else if (nv < 1) code = fail(h, DCFM_ERR_INVALID, "sigma_solve: nv = %d < 1", nv);
    else if (!(tol > 0.0) || !std::isfinite(tol))
        code = fail(h, DCFM_ERR_INVALID, "sigma_solve: tol = %g is not a positive finite number", tol);
    else if (max_iter < 1) code = fail(h, DCFM_ERR_INVALID, "sigma_solve: max_iter = %d < 1", max_iter);
    else if (h->saved < 1) code = fail(h, DCFM_ERR_INVALID, "sigma_solve: no saved sample yet");
    code = sigma_op_enter(h, code, "sigma_solve");
    const size_t P = (size_t)h->d.p;
    const int wmax = std::min<int>(std::max<int>(nv, 1), APPLY_NB);
    ApplyScratch sc;
    SolveEvents ev;
    if (code == DCFM_OK) code = sc.alloc(h, nv, "sigma_solve", SolveMem::doubles(P, wmax));   // before agree(): fails on every rank
    if (int rc = agree(h, code)) {
        sc.release(h);
        return rc;
    }
    if (dev_ms) ev.get(h);
    SolveMem m(sc.more, P, wmax);
    double ms = 0.0;
    int rc = DCFM_OK;
    for (int c0 = 0; c0 < nv && rc == DCFM_OK; c0 += APPLY_NB) {
        const int w = std::min(APPLY_NB, nv - c0);
        rc = solve_chunk(h, sc, m, ev, B + P * c0, w, tol, max_iter, X + P * c0, relres + c0, iters ? iters + c0 : nullptr,
                         quad ? quad + c0 : nullptr, dev_ms ? &ms : nullptr);
    }
    if (rc != DCFM_OK) (void)hipStreamSynchronize(h->stream);   // nothing of the call runs on when the scratch goes
    ev.release(h);
    sc.release(h);
    if (rc == DCFM_OK && dev_ms) *dev_ms = ms;
    return rc;
}
