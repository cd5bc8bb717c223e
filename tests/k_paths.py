"""Census of the code the launchers select from the factor count K, and the cases that reach all of it.

K is the one run-time argument that picks compile-time code (csrc/kernels.hip, csrc/kernels_wide.hip,
csrc/draws.h, csrc/dcfm_internal.h):

  padded width kp                padded_width(K)         32 (K <= 32), 64 (33-64), 128 (65-128)
  narrow loading rows            k_lambda<KE>            KE = 8 (K <= 8), 16 (9-16), 20 (17-20), 24 (21-24),
                                                         30 (25-30), 32 (31-32)
  wide loading rows              k_lambda_w<KW, NB>      NB = ceil(K / 16) = 3, 4 (KW 64), 5, 6, 7, 8 (KW 128)
  wide Z and X draws             k_zdraw / k_xdraw<KW, TK>   TK = ceil(K / 8) = 5 ... 16
  k_draws lanes per row          draw_plan               lrn = lanes_for(ceil(K / 2)), lrg = lanes_for(K),
                                                         lanes_for(c) = 16 (c <= 16), 32 (c <= 32), 64

classes(K) restates that table in plain Python; tests/test_k_paths.py holds it against the launcher text, so a
new instantiation or a moved threshold without a case here fails on the CPU.  CASES are the K values
tests/test_gpu_k_paths.py runs: the lowest and the highest K of every class of every row (from K_MIN on: K = 1
... 7 are tests/test_gpu_parity.py's), one odd K in every narrow class that has one (under an even KE the odd
K leaves one identity-padding row inside the last pivot pair), and so both K = 16 NB (no padding in the last
tile) and K = 16 (NB - 1) + 1 (fifteen padding rows), K = 8 TK and K = 8 (TK - 1) + 1.

Shapes: the smallest that keep every edge live.  g = 2; P = 21 for K <= 32 (two full waves of 8 loading rows
and a partial one of 5), P = 37 for K > 32 (crosses a 32-row residual tile); n = max(40, floor(1.25 K) + 5)
(plus one where that is a multiple of 16), so n > K (the parity regime) and n is ragged
against 16 and 128.  Runs are 3 iterations
(burn-in 1, mcmc 2, thin 1): iteration 1 forms the loading systems from the caller's Plam with Lambda = 0,
iterations 2 and 3 from psi o tau with a real Lambda; two samples are saved.
"""
import functools

K_MIN, K_MAX = 8, 128
G = 2
BURNIN, MCMC, THIN = 1, 2, 1
N_ITER = BURNIN + MCMC
SEED = 5

NARROW = [8, 9, 12, 15, 16, 17, 19, 20, 21, 23, 24, 25, 29, 30, 31, 32]
WIDE = [33, 40, 41, 48, 49, 56, 57, 64, 65, 72, 73, 80, 81, 88, 89, 96, 97, 104, 105, 112, 113, 120, 121, 128]
CASES = NARROW + WIDE
# one K of each class no test reached before (k_lambda<16> against the oracle, k_lambda<24>, k_lambda_w<128, 6>
# with TK 12, TK 14): these also run the guard's fallback and the exact-residual launches
EXTRA_MODE_CASES = [12, 23, 89, 112]

UNFUSED, EXACT, GUARD_ALL = 0x2, 0x10, 0x40     # include/dcfm.h
MODES = {"default": 0, "guard_all": GUARD_ALL, "exact": EXACT}

NARROW_KE = ((8, 8), (16, 16), (20, 20), (24, 24), (30, 30), (32, 32))     # (highest K, KE)


def lanes_for(c):
    return 16 if c <= 16 else (32 if c <= 32 else 64)


def padded_width(K):
    return 32 if K <= 32 else (64 if K <= 64 else 128)


def classes(K):
    """(kp, KE or (KW, NB), TK or None, lrn, lrg): what the launchers select for K = 1 ... 128."""
    if not 1 <= K <= K_MAX:
        raise ValueError(f"K = {K} outside 1 ... {K_MAX}")
    kp = padded_width(K)
    if kp == 32:
        lam = next(ke for top, ke in NARROW_KE if K <= top)
        tk = None
    else:
        lam = (kp, (K + 15) // 16)
        tk = (K + 7) // 8
    return kp, lam, tk, lanes_for((K + 1) // 2), lanes_for(K)


ROWS = ("kp", "lambda", "tk", "lrn", "lrg")


def members(row, lo=K_MIN, hi=K_MAX):
    """{class of table row `row`: the sorted K in lo ... hi that select it} (None, the narrow K's TK, left out)."""
    i = ROWS.index(row)
    out = {}
    for K in range(lo, hi + 1):
        c = classes(K)[i]
        if c is not None:
            out.setdefault(c, []).append(K)
    return out


def shape(K):
    """(n, P, g, K) of the case."""
    n = max(40, (5 * K) // 4 + 5)
    n += n % 16 == 0                     # K = 73 alone: 96 would be whole 16-row tiles; 97 keeps n ragged
    return n, 21 if K <= 32 else 37, G, K


def case_id(K):
    return "K%d" % K


@functools.lru_cache(maxsize=None)
def case(K):
    """helpers.make_case at shape(K): the data, the initial state and the draw source, made once."""
    from helpers import make_case
    n, P, g, _ = shape(K)
    c = make_case(n, P * g, g, K, seed=SEED)
    assert (c["n"], c["P"]) == (n, P), "preprocessing dropped a column"
    return c


# ---- the flat-shrinkage start ---------------------------------------------------------------------------
# At the default start tau_h = prod delta reaches 2e10 and Plam 1e11, so from K ~ 65 on the trailing 16 x 16
# tiles of D Q_j D (D = diag(Q_j)^-1/2) are the identity to rounding: whatever the loading kernels multiply
# there cannot change Lambda (tests/test_loading_measure.py shows it).  The flat start is the case's start
# state with delta = 1, tauh = 1 and Plam = psi (a valid state: Plam = psi o tau), under which every tile of
# the factor carries data (cond(Q_j) <= 310).  It is run for exactly ONE iteration: a second one from it is an
# excursion of the reference itself (max|X| 1.3e4 at K = 33; the oracle's chol fails at K = 40).
FLAT_NARROW = [16, 20, 23, 24, 30, 32]          # one K of every narrow KE class that pairs pivots
FLAT_CASES = FLAT_NARROW + WIDE
FLAT_MODE_CASES = EXTRA_MODE_CASES               # these also under DCFM_FLAG_GUARD_ALL and DCFM_FLAG_EXACT_RESIDUAL
FLAT_ALL = sorted(set(FLAT_CASES) | set(FLAT_MODE_CASES))     # every K the reference is checked at (K = 12 joins)
FLAT_BURNIN, FLAT_MCMC, FLAT_THIN = 0, 1, 1     # the one iteration is the one saved sample


def flat_start(K):
    """The oracle state of case(K)'s start with the shrinkage switched off (a fresh copy)."""
    st = case(K)["st"].copy()
    st.delta[...] = 1.0
    st.tauh[...] = 1.0
    st.Plam[...] = st.psi
    return st


def flat_case(K):
    """case(K) with flat_start(K) as its start state; data, draws and shape are the case's own."""
    c = dict(case(K))
    c["st"] = flat_start(K)
    return c
