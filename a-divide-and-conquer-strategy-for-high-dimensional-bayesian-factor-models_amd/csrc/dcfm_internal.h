// Internal layout + kernel launch declarations for libdcfm (MI355X / gfx950).
//
// HBM layout (C order, last index fastest), G = local shards, mg = global shard,
// KW = d.kp = the padded factor width (32 for K <= 32, 64 for K <= 64, 128 for K <= 128):
//   Y      [G][NP][PP]   standardised data, rows i padded to NP (x16), cols j to PP (x16), zeros
//   yy     [G][PP]       sum_i Y_ij^2 (set_data)                -> residual SS identity
//   Lam    [G][PP][KW]   loadings, k padded to KW with zeros
//   omega  [G][PP]       diag(Omega);   ps [G][PP]
//   psi    [G][PP][KW];  Plam [G][PP][KW] (the caller's Plam; valid until the first
//                        iteration, after which Plam = psi o tau is formed on the fly)
//   X      [NP][KW]      replicated;    Z [G][NP][KW]
//   delta, tau [2][g][KW] replicated on every rank, double-buffered per iteration
//   W      [G][NP][KW]   W_m = Y_m (omega o Lambda_m)  (k_wpass; the fused K <= 32 chain keeps it in
//                        registers: k_wcol draws Z from the W-pass accumulators)
//   A      [G][KW][KW]   A_m = Lambda_m' diag(omega) Lambda_m             (k_prep)
//   ZM     [G][4][KW][KW] Z-draw operators {M1, M2, U, NA} of shard m         (k_prep)
//   Sp     [G][NP][KW]   per-shard X message W_m - sqrt(1-rho) A_m Z_m'   (k_zdraw / k_wcol)
//   xin    [NP][KW]      local sum over shards of Sp;  xall [nranks][NP][KW] all-gathered (== xin if 1 rank;
//                        inside the packed message with the fused several-rank chain, Dims::xstride apart)
//   xa, xa_all [nranks][KW][KW]  per-rank sum of A_m (gathered);  XM [2][KW][KW] X-draw operators {Tx, Ux} (k_xchol)
//   C      [G][PP][KW]   C_m = Y_m' eta_m  (k_cpass);  E [G][KW][KW] = eta_m' eta_m
//   cpart  [G][PP][KW]   psi o Lambda^2 per loading row (k_lambda), summed over rows by k_colsum
//   sloc   [G][KW], sall [g][KW]  column sums (all-gathered)
//   Lb     [2][p][LDB]   saved Lambda rows of an assembly batch (double-buffered), sample s at cols s*K..
//   wsum   [2][p]        sum of saved omega of the batch
//   wslot  [2][p][B]     DCFM_FLAG_SIGMA_M2 / _PRECISION_MEAN / _PARTIAL_CORR / _CORR / _REGRESSION: each saved sample's own omega (slot s of row a at a*B + s)
//   Prec   [ntiles][128][128]  DCFM_FLAG_PRECISION_MEAN: mean of the per-sample Sigma^{-1}, laid out as Sigma
//   pfac   [p][4 KH]     DCFM_FLAG_PRECISION_MEAN / _PARTIAL_CORR / _REGRESSION: the factor panels of a flush (precision_mean.hip), KH = round_up(B K, 16);
//                        pscr [(2 g + 1) B][K][K] the shards' H_m, B_m^{-1} and the slots' S^{-1}
//   PC, PC2 [ntiles][128][128]  DCFM_FLAG_PARTIAL_CORR: mean and second moment of the per-sample partial
//                        correlations, laid out as Sigma (partial_corr.hip; it shares pfac, pscr, wslot)
//   C, C2  [ntiles][128][128]  DCFM_FLAG_CORR: mean and second moment of the per-sample correlation matrix, laid
//                        out as Sigma (corr.hip); cscale [p][B] the rows' 1 / sqrt(Sigma(s)_aa) of a flush,
//                        H, H2 [p] mean and second moment of the communalities
//   Sigma2 [ntiles][128][128]  DCFM_FLAG_SIGMA_M2: second moment of the per-sample Sigma, laid out as Sigma
//   Sigma  [ntiles][128][128]  this rank's block of the lower triangle of Sigmaout, tile-packed:
//                        rank r owns the contiguous tile rows [T0, T1) (balanced by tile count,
//                        sigma_split), tile (ti, tj), tj <= ti, at index tri(ti) - tri(T0) + tj,
//                        inside in k_assemble's accumulator order (sig_tile_off: each lane's two
//                        values of a 16x16 MFMA tile adjacent, so a wave moves the tile with 16-byte
//                        accesses); ~p^2 / (2 nranks) doubles per rank
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcfm {

constexpr int KP = 32;         // padded factor width of the narrow (K <= 32) kernels
constexpr int KP_MAX = 128;    // widest supported padding (K <= 128, config c4 has K = 100)
// padded factor width KW (Dims::kp) of K factors: the kernels are instantiated for these three
constexpr int padded_width(int K) { return K <= 32 ? 32 : (K <= 64 ? 64 : 128); }
constexpr int ASM_TILE = 128;  // covariance-assembly output tile
// Wide paths (KW >= 64) keep E_m = eta_m' eta_m in the loading-row kernel's layout: the
// upper 16x16 tiles (Kc <= I) of the KW/16 x KW/16 tile grid, tile t = etile(KW/16, Kc, I) in
// the fp64 MFMA C/D layout, pair g2 = g / 2 of lane l = c + 16 q at (2t + g2) 128 + 2l + (g & 1)
// for element (16 Kc + q + 4g, 16 I + c) -- one contiguous 16-byte read per lane and pair.
__host__ __device__ constexpr int etile(int nbw, int Kc, int I) { return Kc * nbw - Kc * (Kc - 1) / 2 + (I - Kc); }
__host__ __device__ constexpr int etile_index(int nbw, int R, int Cc) {
    return (2 * etile(nbw, R >> 4, Cc >> 4) + ((R & 15) >> 3)) * 128 + 2 * ((Cc & 15) + 16 * (R & 3)) +
           (((R & 15) >> 2) & 1);
}
constexpr int ASM_KC = 16;            // k_assemble's k chunk (kext, LDB are multiples)
inline int cdiv(int a, int b) { return (a + b - 1) / b; }   // launch grids

struct Dims {
    int n, P, g, K, G;          // G = local shards
    int NP, PP;                 // padded rows / cols
    int shard0;                 // first global shard of this rank
    int nranks, rank;
    int coll;                   // the collective (multi-rank) data path: nranks > 1, or one rank with
                                // a real RCCL communicator (DCFM_FLAG_COMM_SELF)
    int p;                      // P * g
    int kp;                     // padded factor width KW of every [..][KW] array: 32, 64 or 128
    double rho, sr, s1r;        // rho, sqrt(rho), sqrt(1-rho)
    double as_, bs, df, ad1, bd1, ad2, bd2;
    uint64_t seed;
    int inject;
    // gathered-message layout of the fused several-rank chain: the per-rank message is
    // [sloc G x KP | sum_m A_m KP x KP | X message NP x KP] (ONE all-gather per iteration), so
    // rank r's column sums sit at r * xstride, its A sum at that + G*KP and its X message at
    // that + G*KP + KP*KP.  sgap = KP*KP + NP*KP and xstride = G*KP + KP*KP + NP*KP there;
    // sgap = 0, xstride = KW*KW for separate gathers.
    int sgap, xstride;
};

// injected draws on device, [T][...] with T = n_iter of dcfm_set_draws
struct DrawsDev {
    const double *NZ, *NX, *NL, *Gpsi, *Gdelta, *Gps;  // full-g arrays
    int64_t first_iter, n_iter;
};

// loading-row variates of one iteration in k_lambda's layout (local shard m, loading row j):
// NL [G][P][K] (dc:142 zlam), Gpsi [G][P][K] (dc:150), Gps [G][P] (dc:170)
struct LamDraws { const double *NL, *Gpsi, *Gps; };
// dc:180-186 inside k_lambda (K <= 32): where this iteration's sample goes — row a = (shard0 + m) P + j
// of the open batch, Lb[a LDB + slot K + k] = Lambda, wsum[a] += omega, wslot[a B + slot] = omega
// (DCFM_FLAG_SIGMA_M2, else null).  Lb = null: the iteration is not saved, or k_save saves it
struct SaveArgs {
    double *Lb = nullptr, *wsum = nullptr, *wslot = nullptr;
    int LDB = 0, slot = 0, B = 0;
};
// k_wcol's extra blocks generate them for the generated fused chain (K <= 32): one index
// space — [0, n_ps) ps gammas, [n_ps, n_psi) psi gammas, [n_psi, n_all) normal pairs — walked
// grid-stride by b_total blocks of LAM_GEN_THREADS behind the W tiles (VALU work in the slots
// and issue cycles the streaming W pass leaves free)
#ifndef DCFM_LAM_GEN_BLOCKS
#define DCFM_LAM_GEN_BLOCKS 160
#endif
constexpr int LAM_GEN_THREADS = 256, LAM_GEN_BLOCKS = DCFM_LAM_GEN_BLOCKS;
struct LamGen { double *NL, *Gpsi, *Gps; int n_ps, n_psi, n_all, b_total; };
inline int lam_gen_doubles(const Dims &d) { return 2 * d.G * d.P * d.K + d.G * d.P; }
inline LamGen lam_gen_plan(const Dims &d, double *base) {
    const int T = LAM_GEN_THREADS, GP = d.G * d.P;
    LamGen g;
    g.NL = base;
    g.Gpsi = base + (size_t)GP * d.K;
    g.Gps = base + 2 * (size_t)GP * d.K;
    g.n_ps = GP;
    g.n_psi = GP + GP * d.K;
    g.n_all = g.n_psi + GP * ((d.K + 1) / 2);
    const int full = (g.n_all + T - 1) / T;
    g.b_total = full < LAM_GEN_BLOCKS ? full : LAM_GEN_BLOCKS;
    return g;
}

struct Bufs {
    double *Y, *yy, *Lam, *omega, *ps, *psi, *Plam, *X, *Z, *delta, *tau;
    double *ldraw;                     // LamDraws of the generated fused chain (lam_gen_plan), else null
    double *W, *A, *ZM, *Sp, *xin, *xall, *C, *E, *cpart, *sloc, *sall;
    double *Lb[2], *wsum[2], *Sigma;
    double *wslot[2], *Sigma2;         // DCFM_FLAG_SIGMA_M2: per-sample omega of a batch (also with _PRECISION_MEAN),
                                       // second moment; else null
    double *xa, *xa_all, *XM;          // per-rank sum of A, gathered sums, X-draw operators
    double *xpart;                     // k_wcol chunk sums of A (xsum_blocks(G) x KP x KP)
    unsigned *ticket;                  // k_wcol last-arrival ticket (0 between launches)
    unsigned long long *sync;          // hand-off counters (monotonic): [0] = k_xdraw XM out (several ranks),
                                       // [2 + chunk] = k_wcol A_m of the chunk out,
                                       // [SYNC_ZM + m] = k_wcol Z operators of shard m out
    double *msg_all;                   // packed gather target (fused, nranks > 1), else null
    double *agree;                     // 3 doubles: the failure counts of a collective call (comm.hip agree)
    int *rflag;                        // K > 32: [G][PP / 32] 32-row tiles whose SS identity the guard of
                                       // k_lambda_w rejected (k_resid_flagged redoes them and clears the flag)
    int2 *tiles;
    int ntiles, LDB;
    int T0, T1;                        // owned tile rows of Sigma (block-sharded, see above)
};

// This iteration's loading-row variates for this rank's shards.  gen: the buffer k_wcol's extra blocks
// filled (the generated fused chain, K <= 32); else the [T][g][P][K] / [T][g][P] draw buffers dr
// (injected draws, k_draws batches) at iter and the rank's first shard
inline LamDraws lam_draws_at(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, bool gen) {
    if (gen) {
        const LamGen g = lam_gen_plan(d, b.ldraw);
        return {g.NL, g.Gpsi, g.Gps};
    }
    const size_t row0 = ((size_t)(iter - dr.first_iter) * d.g + d.shard0) * d.P;
    return {dr.NL + row0 * d.K, dr.Gpsi + row0 * d.K, dr.Gps + row0};
}

// k_wcol shard sum of A
constexpr int XSUM_BLOCKS = 8;
constexpr int TRACE_SLICES = 16;       // k_trace_part blocks per local shard (slices of its loading rows)
// Probe draws (probes.hip): at most PROBE_NV_MAX probe vectors; k_probes runs probe_slices(G) blocks per
// local shard, each a fixed slice of its loading rows: about one block per CU, so that a few big shards
// (c4: 8 of 1250 rows, K = 100) are split 32 ways and many small ones (c3: 64 of 312 rows) only 4 ways --
// a slice's partial is K nv + nv^2 doubles, more than the ~10 rows a 32-way slice of c3 would read
constexpr int PROBE_NV_MAX = 32, PROBE_SLICES_MAX = 32, PROBE_FAN = 8;   // FAN: shard terms added per group
inline int probe_slices(int G) { return G >= 256 ? 1 : (256 / G < PROBE_SLICES_MAX ? 256 / G : PROBE_SLICES_MAX); }
// device buffers of dcfm_set_probes: V [G * P][nv] this rank's rows of the probe block (row-major),
// part [G][slices][ts] slice partials, term [G][ts] shard terms and gterm [ceil(G / PROBE_FAN)][ts] group
// sums, each [W (K x nv) | D (nv x nv)] with ts = K nv + nv^2, ticket: last-arrival tickets of the
// shards, the groups and the rank, draws [capacity][slot]:
// slot = nv^2 (one rank: V' Sigma(s) V itself) or ts (several ranks: [W_r | D_r])
struct Probes {
    const double *V;
    double *part, *term, *gterm, *draws;
    unsigned *ticket;
    int nv, slices;
    size_t slot;
};
// Precision draws (precision.hip): V' Sigma(s)^{-1} V and log det Sigma(s) per saved sample.  k_precision runs
// precision_slices blocks per local shard; a slice's partial is the lower 16x16 tiles of the weighted Gram of
// [Lambda_m | V_m] (wp^2 / 2 doubles, wp = K + nv padded to 16), so a slice reads at least wp / 2 rows
__host__ __device__ constexpr int precision_tiles(int K, int nv) { return ((K + nv + 15) / 16) * ((K + nv + 15) / 16 + 1) / 2; }
inline int precision_slices(int G, int P, int K, int nv) {
    const int wp = (K + nv + 15) / 16 * 16, rows = wp / 2 > 8 ? wp / 2 : 8, cap = P / rows > 1 ? P / rows : 1;
    return probe_slices(G) < cap ? probe_slices(G) : cap;
}
// device buffers of dcfm_set_precision_probes, w = K + nv: V [G * P][nv] as Probes::V, part [G][slices][ps] slice
// partials (ps = 256 precision_tiles + 1: the tiles in the MFMA C/D layout, then sum log omega), gram [G][w][w]
// the shards' folded Gram (both triangles), term [G][ts] shard terms, gterm [ceil(G / PROBE_FAN)][ts] group sums
// and rsum [ts] the rank's sum, each [H | F (K x w, row-major) | q (nv x nv) | ld] with ts = K w + nv^2 + 1,
// xs [K][nv] the solve S^{-1} F, ticket as Probes::ticket, draws [capacity][slot]: slot = nv^2 + 1 (one rank:
// the draw and its log det) or ts (several ranks: the rank's sum)
struct Precision {
    const double *V;
    double *part, *gram, *term, *gterm, *rsum, *xs, *draws;
    unsigned *ticket;
    int nv, slices;
    size_t slot, lds;
};
// Pointwise log-likelihood draws (loglik.hip): y_i' Sigma(s)^{-1} y_i of every training row and log det Sigma(s)
// per saved sample.  pr: k_precision's scratch at nv = 0 (no V, no draws); T [G][NP][KW] the pass T_m = Y_m
// Omega_m^{-1} Lambda_m and sq [G][NP] its row sums s_m (k_loglik_shard turns them in place into F_m = T_m B_m^{-1}
// and the shards' terms s_m - (1 - rho) t.f); binv [G][K][K] the shards' B_m^{-1}; hsum [K K + 1] the
// rank's [H_r | ld_r]; sinv [K K + 1] = [S^{-1} | log det Sigma] (one rank); draws [capacity][slot]: slot = n + 1
// (one rank: [q | ld]) or n K + n + K K + 1 (several ranks: [U_r (n x K) | q_r | H_r | ld_r]); lds: k_loglik_close's
// dynamic LDS bytes
struct LogLik {
    Precision pr;
    double *T, *sq, *binv, *hsum, *sinv, *draws;
    size_t slot, lds;
};
// Conditional prediction (predict.hip): pr k_precision's scratch at nv = T with pr.V = the new rows Y* [G P][T]
// (row-major, the unobserved entries zero; no pr.draws); obs [G P] the 0 / 1 mask; sinv [K][K] = S^{-1} and qd
// [T T + 1] = [q | ld] of the sample in flight; work [G][4 K K + 2 K T] the K x K products of k_predict_prod; coef
// [G][K4][wc] = [t_m (Tp columns) | N_m (16 ceil(K / 16))] zero-padded, K4 = K rounded up to 4, Tp = T to 16;
// the accumulators sum, sum2 [G P][T] and cvsum [G P]; draws [capacity][T + 1] = [diag q | ld]
struct Predict {
    Precision pr;
    unsigned char *obs;
    double *sinv, *qd, *work, *coef, *sum, *sum2, *cvsum, *draws;
    int T, Tp, wc;
};
// Missing training data (impute.hip, dcfm_set_missing; nmiss == 0 when off).  The nmiss missing entries of this
// rank's shards are listed twice: as entries e sorted by (local shard, row i, column j) -- row[e] = i, col[e] = m PP + j
// (the index into yy / ps), perm[e] = the entry's place in the second order -- and as vcsc, their current values
// sorted by (local shard, column, row), where column c of the ncol columns with a missing entry (cols[c] = m PP + j)
// owns vcsc[colptr[c] .. colptr[c + 1]).  yyobs [ncol] = the sum of squares of a column's observed entries.  The
// accumulators of dcfm_get_imputed (null with capacity 0): smu, smu2 [nmiss] in entry order, snv [ncol]
struct Impute {
    int nmiss, ncol;
    const int *row, *col, *perm, *colptr, *cols;
    double *vcsc, *yyobs, *smu, *smu2, *snv;
};
// Precision mean (precision_mean.hip, DCFM_FLAG_PRECISION_MEAN; all null when off).  Kept out of Bufs, which
// the sweep's kernels take by value: Prec the accumulator (laid out as Bufs::Sigma), pfac the factor panels of
// a flush, pscr the K x K scratch, KH the columns of a quarter of pfac (B K rounded up to ASM_KC).
// DCFM_FLAG_PARTIAL_CORR or DCFM_FLAG_REGRESSION alone allocates pfac and pscr (the panel stage is shared) and
// leaves Prec null
struct PrecMean {
    double *Prec, *pfac, *pscr;
    int KH;
};
// Partial correlations (partial_corr.hip, DCFM_FLAG_PARTIAL_CORR; null when off): PC the mean and PC2 the second
// moment of the per-sample R(s), both laid out as Bufs::Sigma
struct PartialCorr {
    double *PC, *PC2;
};
// Marginal correlations and communalities (corr.hip, DCFM_FLAG_CORR; all null when off): C the mean and C2 the
// second moment of the per-sample R(s), both laid out as Bufs::Sigma; cscale [p][B] the scales of a flush;
// H, H2 [p] the two moments of the communalities (all p rows on every rank)
struct Corr {
    double *C, *C2, *cscale, *H, *H2;
};
// Regression coefficients (regression.hip, DCFM_FLAG_REGRESSION with dcfm_set_regression; q == 0 when off), passed
// to its kernels by value.  resp [q] the response rows; the nsh distinct shards that hold one are numbered
// ascending: tof [g] a shard's number or -1, grp [q] the responses' positions in R grouped by shard number (R's
// order inside a group), goff [nsh + 1] the groups' starts.  scr [B][sstride] the slots' scratch: [C (q q) | R2 (q)]
// and, wofs doubles in, [W_G | W_A[0] .. W_A[nsh - 1]], each K4 x qp row-major (K4 = K rounded up to 4, qp = q to
// 16; the padding stays the zero it was allocated as).  The accumulators: sB, sB2 [p][q] row-major, sC, sC2
// [q q + q] = the sums of [C | R2] and of their squares
struct Regress {
    int q, qp, nsh, K4;
    const int *resp, *grp, *goff, *tof;
    double *scr;
    size_t sstride, wofs;
    double *sB, *sB2, *sC, *sC2;
};
// Bufs::sync: [0] the X operators (k_xdraw, several ranks), [1] spare, [2, 2 + 256) chunk counters of the A sum, [SYNC_ZM, SYNC_ZM + G) the
// per-shard Z-operator counters (the fused W pass draws Z once its shard's operators are out)
constexpr int SYNC_ZM = 2 + 256;
// blocks of the A sum: G / chunk, chunk = a power of two dividing G, grown while more than
// XSUM_BLOCKS chunks remain — so each chunk is a subtree of the canonical tree (TreeSum) and
// the tree over the chunk sums is T(0, G).  G <= XSUM_BLOCKS: one block sums every shard
// (tree8 with zero padding is T(0, G)), without the chunk-sum hand-off round
__host__ __device__ inline int xsum_blocks(int G) {
    if (G <= XSUM_BLOCKS) return 1;
    int chunk = 1;
    while (G / chunk > XSUM_BLOCKS && (G / chunk) % 2 == 0) chunk *= 2;
    return G / chunk;
}

// Sigma block-sharding helpers (host + device)
__host__ __device__ inline long long tri(long long t) { return t * (t + 1) / 2; }
// offset of the stored element (a, b), a >= b, in a rank's tile-packed Sigma (owner of tile row a/128)
// Inside a tile, element (ra, cb) sits where k_assemble's wave w = 2 (ra / 64) + cb / 64 holds it
// in the f64 MFMA C/D layout: 16x16 tile (u, v) = ((ra / 16) % 4, (cb / 16) % 4), row ra % 16 =
// q + 4 g, lane q * 16 + cb % 16; the lane's values g = 2 h, 2 h + 1 are adjacent, so a wave moves
// one (u, v, h) slice as one 16-byte access per lane, 1 KiB contiguous
__host__ __device__ inline int sig_tile_off(int u, int v, int g, int w, int lane) {
    return ((((w * 4 + u) * 4 + v) * 2 + (g >> 1)) * 64 + lane) * 2 + (g & 1);
}
__host__ __device__ inline size_t sig_off(int a, int b, int T0) {
    const int ta = a / ASM_TILE, tb = b / ASM_TILE, ra = a % ASM_TILE, cb = b % ASM_TILE, rr = ra & 15;
    return (size_t)(tri(ta) - tri(T0) + tb) * ASM_TILE * ASM_TILE +
           sig_tile_off((ra >> 4) & 3, (cb >> 4) & 3, rr >> 2, 2 * (ra >> 6) + (cb >> 6), (rr & 3) * 16 + (cb & 15));
}
// Packed window of a rank owning rows [R0, R1) in a column stripe: column c holds the rows
// [lo(c), R1) of Sigmaout(:, c) it owns (lo = 0 for c in [R0, R1): the upper part mirrored from
// its own rows; lo = R0 for c < R0; nothing for c >= R1).  off(c) = start of column c in the
// rank's packed stripe [c0, ...).
__host__ __device__ inline long long win_lo(long long c, long long R0, long long R1) {
    return (c >= R0 && c < R1) ? 0 : (c < R0 ? R0 : R1);
}
__host__ __device__ inline long long win_off(long long c, long long c0, long long R0, long long R1) {
    const long long na = (c < R0 ? c : R0) - c0;                 // columns of [c0, c) below R0
    const long long b0 = c0 > R0 ? c0 : R0, b1 = c < R1 ? c : R1;  // columns of [c0, c) in [R0, R1)
    return (na > 0 ? na : 0) * (R1 - R0) + (b1 > b0 ? b1 - b0 : 0) * R1;
}

// launchers of the sweep (kernels.hip; K > 32 forwards to wide:: where the kernels differ)
void launch_prep(const Dims &d, const Bufs &b, hipStream_t s);
void launch_wpass(const Dims &d, const Bufs &b, hipStream_t s);
void launch_zdraw(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, hipStream_t s);
void launch_xred(const Dims &d, const Bufs &b, hipStream_t s);
// fused K <= 32 launches (kernels.hip: the roles of k_wcol, k_xdraw and k_cpass)
// K <= 32: the Z operators + shard sum of A (ops), the previous iteration's column sums
// (colsum) and the Y pass W with the Z draw of its rows (wpass: Z, Sp; needs ops) in one launch
// (k_wcol); one rank also factors Xprec
void launch_wcol(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, bool ops, bool colsum, bool wpass,
                 unsigned long long ops_epoch, hipStream_t s, bool lamgen = false);
// several ranks, K <= 32: k_xdraw with the X operators (block 0, from the ranks' A sums of the
// packed gather, published through the counter b.sync[0] at xm_epoch) and the row blocks
// summing the ranks' X messages
void launch_xdraw_mr(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, unsigned long long xm_epoch,
                     hipStream_t s);
void launch_asum(const Dims &d, const Bufs &b, hipStream_t s);
void launch_xchol(const Dims &d, const Bufs &b, hipStream_t s);
void launch_xdraw(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, hipStream_t s,
                  bool from_shards = false);
// k_cpass; with delta_in (fused K <= 32 chain) also the delta / tau chain of delta_iter in
// extra blocks (column sums from b.sall)
void launch_cpass(const Dims &d, const Bufs &b, hipStream_t s, const DrawsDev &dr = DrawsDev{},
                  const double *delta_in = nullptr, const double *tau_in = nullptr, double *delta_out = nullptr,
                  double *tau_out = nullptr, int64_t delta_iter = 0);
// gen: lam_draws_at.  kappa_max: a row whose SS identity may be off by more than ~kappa_max eps (the
// guard, resid.h) takes ps, omega from dc:169's direct residual instead: K <= 32 its wave's 8 rows in
// the same launch, K > 32 its 32-row tile in launch_resid_flagged.  sv (K <= 32 only): the kernel also
// saves the sample
void launch_lambda(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter,
                   const double *tau_cur, const double *plam_src, hipStream_t s, bool gen, double kappa_max,
                   const SaveArgs &sv = SaveArgs{});
void launch_colsum(const Dims &d, const Bufs &b, hipStream_t s);
// resid.hip (DCFM_FLAG_EXACT_RESIDUAL): ps, omega from the direct residual Yd - eta Lambda' (dc:169-171)
// for every loading row, after the loading-row kernel, with its ps variates (gen: b.ldraw, else dr)
void launch_resid(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, hipStream_t s, bool gen);
// K > 32, default mode: the same for the 32-row tiles k_lambda_w's guard flagged (b.rflag); the other
// blocks exit at once
void launch_resid_flagged(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, hipStream_t s);
void launch_delta(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter,
                  const double *delta_in, const double *tau_in, double *delta_out,
                  double *tau_out, hipStream_t s);
// assemble.hip: saved samples of a batch, their accumulation into Sigma, the output stripes
// (wslot, DCFM_FLAG_SIGMA_M2: also the sample's omega into slot `slot` of B)
void launch_save(const Dims &d, const Bufs &b, double *Lb, double *wsum, int slot, hipStream_t s,
                 double *wslot = nullptr, int B = 0);
void launch_assemble(const Dims &d, const Bufs &b, const double *Lb, const double *wsum, int kext,
                     double inv_eff, hipStream_t s);
// assemble_m2.hip: b.Sigma2 += (1 / effsamp) sum over the batch's nslots samples of the squared
// per-sample Sigma (Lb slots of K columns, wslot [p][B] the samples' omega)
void launch_assemble_m2(const Dims &d, const Bufs &b, const double *Lb, const double *wslot, int nslots, int B,
                        double inv_eff, hipStream_t s);
// precision_mean.hip: pm.Prec += (1 / effsamp) sum over the batch's nslots samples of Sigma(s)^{-1}, from the
// gathered Lb slots and wslot [p][B] of ALL g shards; setup once per process before the first launch.
// launch_precision_panels: the panel stage (k_pm_shard, k_pm_s, k_pm_panels) into pm.pfac, once per flush for the
// precision mean and the partial correlations; launch_precision_mean: the two accumulation passes behind it
size_t precision_mean_scratch_doubles(int g, int K, int B);
hipError_t precision_mean_setup();
void launch_precision_panels(const Dims &d, const Bufs &b, const PrecMean &pm, const double *Lb, const double *wslot,
                             int nslots, int B, hipStream_t s);
void launch_precision_mean(const Dims &d, const Bufs &b, const PrecMean &pm, const double *wslot, int nslots, int B,
                           double inv_eff, hipStream_t s);
// the same tile loop over panels scaled per row by k_pc_scale: PC += (1 / effsamp) sum_s R(s), the off-diagonal
// sign +, the diagonal exactly nslots / effsamp (G pass, then A pass)
void launch_pc_mean(const Dims &d, const Bufs &b, const PrecMean &pm, int nslots, double inv_eff, double *PC,
                    hipStream_t s);
// partial_corr.hip, behind launch_precision_mean on the same stream: scales pm.pfac in place (k_pc_scale), then
// pc.PC += (1 / effsamp) sum_s R(s) and pc.PC2 += (1 / effsamp) sum_s R(s).^2 over the batch's nslots samples
void launch_partial_corr(const Dims &d, const Bufs &b, const PrecMean &pm, const PartialCorr &pc, const double *wslot,
                         int nslots, int B, double inv_eff, hipStream_t s);
// regression.hip, behind launch_precision_panels and BEFORE launch_partial_corr (which scales pm.pfac in place) on
// the same stream: the batch's nslots samples one by one, in slot order, into rg's six sums; pm.pfac, Lb and wslot
// are only read
void launch_regression(const Dims &d, const Bufs &b, const PrecMean &pm, const Regress &rg, const double *Lb,
                       const double *wslot, int nslots, int B, hipStream_t s);
// corr.hip, on the assembly stream: cr.cscale and cr.H / cr.H2 of the batch's nslots samples (k_corr_scale), then
// cr.C += (1 / effsamp) sum_s R(s) and cr.C2 += (1 / effsamp) sum_s R(s).^2 (k_corr); Lb and wslot are only read
void launch_corr(const Dims &d, const Bufs &b, const Corr &cr, const double *Lb, const double *wslot, int nslots,
                 int B, double inv_eff, hipStream_t s);
// column stripe [c0, c0 + nc) of Sigmaout from a rank's tile-packed block (tile rows [T0, T1)):
// the rank's packed windows (win_lo / win_off; with one rank = the dense p x nc stripe).
// which (DCFM_SIGMA_*): 0 the mean S, 1 the second moment S2, 2 sqrt(max(0, rs S2 - (rs S)^2)).
// diag (host pointer, nullable): the value written on the diagonal instead of the one read
void launch_sigma_pack(const double *S, const double *S2, int which, double rs, int p, int T0, int T1, int c0,
                       int nc, double *out, hipStream_t s, const double *diag = nullptr);
// root of the gather: the dense p x nc stripe from every rank's packed windows, rank k's at
// recv + base[k]; Tb[0..nranks] are the ranks' tile-row boundaries (device arrays)
void launch_sigma_unpack(const double *recv, int p, int c0, int nc, const int *Tb, const long long *base,
                         int nranks, double *out, hipStream_t s);
// kernels.hip: eta = sqrt(rho) X + sqrt(1-rho) Z for every local shard (K > 32: once per iteration)
void launch_eta(const Dims &d, const Bufs &b, double *eta_out, hipStream_t s);
// sigma_err.hip: rows' sums of (Sigmaout - U U' - diag s) v, squares and truth squares
// (partials [splits][p] in y / fro / tru; summed into out[0..p), out[p..2p), out[2p..3p))
int sigma_err_splits(int p);
void launch_sigma_err(const double *S, int p, const double *U, int R, const double *sdiag, const double *v,
                      int T0, int T1, bool first, double *y, double *fro, double *tru, double *out,
                      hipStream_t s);
// sigma_apply.hip: Y (p x nv column-major, nv <= 32) = this rank's tile rows [T0, T1) of the mirrored
// Sigmaout times V (p x nv column-major); each stored tile read once.  scratch: sigma_apply_scratch
// doubles (the tiles' partial panels, summed in a fixed order by a second kernel)
size_t sigma_apply_scratch(int T0, int T1, int nv);
void launch_sigma_apply(const double *S, int p, int T0, int T1, const double *V, int nv, double *scratch, double *Y,
                        hipStream_t s);
// ingest.hip: dc:31-34 column nnz counts; dc:50-59 partition + standardise into Y / yy
void launch_nnz_cols(const double *Y, int n, long long p, int *nnz, hipStream_t s);
void launch_stdize(const Dims &d, const double *Yraw, const long long *cols, double *Y, double *yy, double *sd,
                   int *bad, double *mean_inv, hipStream_t s);
// trace.hip: per-iteration chain summaries (||Lambda||_F^2, tr Omega, sum log ps, sum log tau) into
// row [G][4]; scratch = trace_scratch_doubles(G) zeroed doubles (slice partials + per-shard tickets)
inline size_t trace_scratch_doubles(int G) { return (size_t)G * TRACE_SLICES * 4 + (G + 1) / 2; }
void launch_trace(const Dims &d, const Bufs &b, const double *tau_cur, double *scratch, double *row, hipStream_t s);
// probes.hip: draw s of V' Sigma V from the current Lambda, omega (after launch_save, same stream)
void launch_probes(const Dims &d, const Bufs &b, const Probes &pr, int64_t s, hipStream_t st);
// precision.hip: draw s of V' Sigma^{-1} V and log det Sigma from the current Lambda, omega (same place)
void launch_precision(const Dims &d, const Bufs &b, const Precision &pr, int64_t s, hipStream_t st);
// the same kernel at nv = 0 for loglik.hip: out [K K + 1] = the rank's sum [H_r | ld_r], binv [G][K][K] the
// shards' B_m^{-1}.  Its scratch: precision_scratch_doubles doubles, the first precision_ticket_doubles zeroed
// by the caller, laid out by precision_scratch_carve (which fills pr but V and draws); precision_setup once
// before the first launch (the kernel's dynamic-LDS limit)
void launch_precision_terms(const Dims &d, const Bufs &b, const Precision &pr, double *binv, double *out, hipStream_t st);
size_t precision_ticket_doubles(const Dims &d);
size_t precision_scratch_doubles(const Dims &d, int nv);
void precision_scratch_carve(const Dims &d, int nv, double *mem, Precision &pr);
hipError_t precision_setup();
// the one-rank form with the Gram's weight masked by obs [G][P] (an unobserved row: weight 0, log term 0) and pr.V
// the new rows: draw = [q (nv x nv) | ld] of Sigma_AA, sinv [K][K] = S^{-1}; pr.term, pr.rsum, pr.xs are left holding
// [H_m | F_m], [H | F] and S^{-1} F
void launch_precision_masked(const Dims &d, const Bufs &b, const Precision &pr, const unsigned char *obs, double *sinv,
                             double *draw, hipStream_t st);
// predict.hip: sample s of the conditional prediction from the current Lambda, omega (same place, one rank)
void launch_predict(const Dims &d, const Bufs &b, const Predict &pd, int64_t s, hipStream_t st);
// impute.hip: the data-augmentation step of iteration iter from the final X, Z, Lambda, ps (k_impute: the missing
// entries of Y and vcsc redrawn; k_impute_yy: yy of their columns); acc: also one sample into the accumulators
void launch_impute(const Dims &d, const Bufs &b, const Impute &im, int64_t iter, bool acc, hipStream_t s);
// loglik.hip: draw s of the rows' y_i' Sigma^{-1} y_i and log det Sigma from the current Lambda, omega (same place)
void launch_loglik(const Dims &d, const Bufs &b, const LogLik &ll, int64_t s, hipStream_t st);
// init.hip: dc:68-87 initial state from Philox (iteration-0 counters), delta/tau buffer 0
void launch_init_state(const Dims &d, const Bufs &b, hipStream_t s);
// kernels.hip: one iteration's variates into the draw buffers (side-stream layouts)
void launch_draws(const Dims &d, const DrawsDev &dr, int64_t iter, hipStream_t s);
// NaN / Inf sentinel over the state (sets *flag = 1 if any value is non-finite)
void launch_finite(const Dims &d, const Bufs &b, const double *tau_cur, int *flag, hipStream_t s);
// dst[i] = sum_k src[k * count + i] in slice order (loopback all-reduce)
void launch_sum_slices(const double *src, int ns, size_t count, double *dst, hipStream_t s);
void launch_rng_fill(uint64_t seed, int kind, double shape, int site, int shard, int64_t iter,
                     int64_t count, int width, double *out, hipStream_t s);

// wide-factor kernels (kp = 64 / 128; kernels_wide.hip), dispatched from the launchers above
namespace wide {
void launch_prep(const Dims &d, const Bufs &b, hipStream_t s);
void launch_xchol(const Dims &d, const Bufs &b, hipStream_t s);
void launch_zdraw(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, hipStream_t s);
void launch_xdraw(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, hipStream_t s);
void launch_lambda(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, const double *tau_cur,
                   const double *plam_src, hipStream_t s, double kappa_max);
void launch_delta(const Dims &d, const Bufs &b, const DrawsDev &dr, int64_t iter, const double *delta_in,
                  const double *tau_in, double *delta_out, double *tau_out, hipStream_t s);
}  // namespace wide

}  // namespace dcfm
