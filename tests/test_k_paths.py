"""The census of K-selected code (tests/k_paths.py) against the launcher text, the coverage of its case list,
and the reference at every case.  No GPU.

  1. classes(K) is what the launchers instantiate: the LAUNCH_LAM(..) thresholds of kernels.hip, the
     LT(KW, NB) cases and dispatch_tk's range of kernels_wide.hip, padded_width of dcfm_internal.h and
     draw_plan's lanes_for of draws.h are read from the source, K = 1 ... 128 is run through what was read, and
     the result must be classes(K).  The instantiated (KE), (KW, NB) and (KW, TK) sets must be exactly the
     census's classes: a new instantiation or a moved threshold without a case fails here.
  2. CASES holds the lowest and the highest K of every class of every row, and an odd K of every narrow
     loading-row class that has one.
  3. The reference is well posed at every case.  Whole-chain runs of the two oracle flavours are no bar at these
     shapes: after two iterations they differ by up to 2.6e-7 at K = 128, n = 165 (the ill-conditioning DESIGN.md
     section 2 describes).  The stage-wise comparison is: the faithful loop's iteration from a given start,
     measured with helpers.stagewise_errors (the vectorised restatement, stage by stage, from that same start)
     -- the same measurement the GPU test makes of the library.  Condition: <= 1e-12 on every field, loading
     backward error <= 1e-15, ps and omega finite and positive.  A case that misses it gets another n, not
     another bar.
  4. The same at the flat start (k_paths.flat_case: delta = 1, tauh = 1, Plam = psi; one iteration, never
     continued), where cond(Q_j) <= 310 makes a forward bar legitimate: the two flavours' Lambda agree to 1e-12
     normwise, max|X| stays in the stationary range, and the case list has one K of every narrow class that
     pairs pivots and every wide case.  The diagonally scaled loading measure, its bars and what the flat start
     reaches are tests/test_loading_measure.py's.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import k_paths as kp
from oracle import dc_oracle as F

CSRC = next(Path(__file__).resolve().parents[1].glob("*_amd")) / "csrc"

SELF_TOL = 1e-12      # faithful loop vs the vectorised stages, from the same start
SELF_BW = 1e-15       # the faithful loop's own loading backward error
FLAT_COND = 1e3       # cond(Q_j) at the flat start (measured <= 306, K = 88)
FLAT_XMAX = 10.0      # max|X| after the flat start's one iteration (measured <= 3.04)


def _text(name):
    return (CSRC / name).read_text()


def _ternary_steps(expr):
    """'c <= 16 ? 16 : (c <= 32 ? 32 : 64)' -> ([(16, 16), (32, 32)], 64)."""
    steps = [(int(a), int(b)) for a, b in re.findall(r"\w+ <= (\d+) \? (\d+) :", expr)]
    last = int(re.search(r": (\d+)\)*\s*;?\s*$", expr.strip()).group(1))
    assert steps, expr
    return steps, last


def _step(steps_last, v):
    steps, last = steps_last
    return next((out for top, out in steps if v <= top), last)


def _source_census():
    """What the launcher text selects: a function K -> classes tuple, and the instantiated sets."""
    internal, narrow, wide, draws = (_text(f) for f in ("dcfm_internal.h", "kernels.hip", "kernels_wide.hip", "draws.h"))
    kp_narrow = int(re.search(r"constexpr int KP = (\d+);", internal).group(1))
    kp_max = int(re.search(r"constexpr int KP_MAX = (\d+);", internal).group(1))
    pw = _ternary_steps(re.search(r"constexpr int padded_width\(int K\) \{ return (.*?); \}", internal).group(1))
    lf = _ternary_steps(re.search(r"inline int lanes_for\(int c\) \{ return (.*?); \}", draws).group(1))
    assert re.search(r"const int kp2 = \(d\.K \+ 1\) / 2;\s*pl\.lrn = lanes_for\(kp2\);\s*pl\.lrg = lanes_for\(d\.K\);", draws)

    # narrow loading rows: the if / else-if chain between #define LAUNCH_LAM and #undef LAUNCH_LAM
    body = narrow[narrow.index("#define LAUNCH_LAM(KE)"):narrow.index("#undef LAUNCH_LAM")]
    assert "if (d.kp != KP) return wide::launch_lambda(" in narrow
    chain = re.findall(r"(?:else )?if \(d\.K <= (\d+)\) LAUNCH_LAM\((\d+)\);", body)
    tail = re.findall(r"else LAUNCH_LAM\((\d+)\);", body)
    uses = re.findall(r"LAUNCH_LAM\((\d+)\)", body)
    assert len(tail) == 1 and len(uses) == len(chain) + 1, "a LAUNCH_LAM(..) use this test does not read"
    lam_n = ([(int(a), int(b)) for a, b in chain], int(tail[0]))
    assert [a for a, _ in lam_n[0]] == sorted(a for a, _ in lam_n[0])

    # wide loading rows: switch ((d.K + 15) / 16) over LT(KW, NB)
    body = wide[wide.index("#define LT(KWV, NBV)"):wide.index("#undef LT")]
    assert "switch ((d.K + 15) / 16)" in body
    cases = {int(c): (int(w), int(nb)) for c, w, nb in re.findall(r"case (\d+): LT\((\d+), (\d+)\); break;", body)}
    default = tuple(int(x) for x in re.search(r"default: LT\((\d+), (\d+)\); break;", body).groups())
    assert len(re.findall(r"\bLT\(\d+, \d+\)", body)) == len(cases) + 1, "an LT(..) use this test does not read"

    # wide draws: tk = (K + 7) / 8, instantiated for KW / 16 + 1 ... KW / 8 of KW = 64 and 128
    assert re.search(r"dispatch_tk_impl<KW>\(\(K \+ 7\) / 8, f, std::make_integer_sequence<int, KW / 16>\{\}\);", wide)
    assert "((tk == KW / 16 + 1 + I ? (f(std::integral_constant<int, KW / 16 + 1 + I>{}), 0) : 0), ...);" in wide
    widths = sorted(int(w) for w in set(re.findall(r"constexpr int KW = (\d+);", wide[wide.index("#define WIDE_DISPATCH"):
                                                                                     wide.index("void launch_prep")])))
    tk_inst = {(w, w // 16 + 1 + i) for w in widths for i in range(w // 16)}

    def select(K):
        kpw = _step(pw, K)
        if kpw == kp_narrow:
            lam, tk = _step(lam_n, K), None
        else:
            nb = (K + 15) // 16
            lam = cases.get(nb, default)
            tk = (K + 7) // 8
            assert lam[0] == kpw, f"K = {K}: k_lambda_w<{lam[0]}, ..> on buffers padded to {kpw}"
            assert (kpw, tk) in tk_inst, f"K = {K}: no k_zdraw / k_xdraw<{kpw}, {tk}>"
        return kpw, lam, tk, _step(lf, (K + 1) // 2), _step(lf, K)

    inst = dict(ke={b for _, b in lam_n[0]} | {lam_n[1]}, lt=set(cases.values()) | {default}, tk=tk_inst,
                kp_max=kp_max, widths=widths)
    return select, inst


def test_census_matches_the_launchers():
    select, inst = _source_census()
    assert inst["kp_max"] == kp.K_MAX
    for K in range(1, kp.K_MAX + 1):
        assert kp.classes(K) == select(K), f"K = {K}: census {kp.classes(K)}, launchers {select(K)}"
    # every instantiation is a class of the census, and the other way round
    lam = set(kp.members("lambda", 1))
    assert inst["ke"] == {c for c in lam if isinstance(c, int)}
    assert inst["lt"] == {c for c in lam if isinstance(c, tuple)}
    assert inst["tk"] == {(kp.padded_width(Ks[0]), tk) for tk, Ks in kp.members("tk", 1).items()}
    assert set(kp.members("kp", 1)) == {32} | set(inst["widths"])
    with pytest.raises(ValueError):
        kp.classes(kp.K_MAX + 1)


def test_cases_cover_every_class():
    assert kp.CASES == sorted(set(kp.CASES)) and kp.K_MIN <= kp.CASES[0] and kp.CASES[-1] <= kp.K_MAX
    assert set(kp.EXTRA_MODE_CASES) <= set(kp.CASES)
    for row in kp.ROWS:
        for cls, Ks in kp.members(row).items():
            assert Ks[0] in kp.CASES and Ks[-1] in kp.CASES, f"{row} class {cls}: K = {Ks[0]} ... {Ks[-1]} lacks an end"
    for ke, Ks in kp.members("lambda", kp.K_MIN, 32).items():
        odd = [K for K in Ks if K % 2]
        assert not odd or set(odd) & set(kp.CASES), f"k_lambda<{ke}>: no odd K among the cases"
    # the edges inside a class, spelled out
    for nb in range(3, 9):
        assert 16 * nb in kp.CASES and 16 * (nb - 1) + 1 in kp.CASES
    for tk in range(5, 17):
        assert 8 * tk in kp.CASES and 8 * (tk - 1) + 1 in kp.CASES
    for K in (16, 17, 32, 33, 64, 65):              # draw_plan's lane steps
        assert K in kp.CASES
    # the classes the suite did not reach before
    assert kp.classes(12)[1] == 16 and kp.classes(23)[1] == 24
    assert kp.classes(89)[1:3] == ((128, 6), 12) and kp.classes(112)[2] == 14


def test_shapes():
    for K in kp.CASES:
        n, P, g, _ = kp.shape(K)
        assert n > K and n % 16 and n % 128 and g == 2
        assert (P % 8 and P > 16) if K <= 32 else (P % 32 and P > 32)


@pytest.mark.parametrize("K", kp.CASES, ids=kp.case_id)
def test_reference_is_well_posed(K):
    from helpers import stagewise_errors
    c = kp.case(K)
    ref = c["st"].copy()
    assert not np.any(ref.Lambda), "iteration 1 starts from Lambda = 0 with the caller's Plam"
    worst, worst_bw = {}, 0.0
    for it in range(1, kp.N_ITER + 1):
        start = ref.copy()
        dr = c["src"].iteration(it)
        F.gibbs_iteration(ref, c["Yd"], c["rho"], c["hyper"], dr)
        errs, bw, _ = stagewise_errors(start, ref.as_dict(), c["Yd"], c["rho"], c["hyper"], dr)
        for f in ("ps", "omega"):
            v = getattr(ref, f)
            assert np.all(np.isfinite(v)) and np.all(v > 0.0), f"K = {K} iteration {it}: reference {f} out of range"
        for f, e in errs.items():
            worst[f] = max(worst.get(f, 0.0), e)
        worst_bw = max(worst_bw, bw)
    print("K_PATHS_REFERENCE", kp.case_id(K), kp.shape(K), {f: f"{e:.2e}" for f, e in sorted(worst.items())},
          f"lambda_bw {worst_bw:.2e}")
    for f, e in worst.items():
        assert e <= SELF_TOL, f"K = {K}: the oracle's two flavours differ in {f} by {e:.3e} (bar {SELF_TOL:.0e})"
    assert worst_bw <= SELF_BW, f"K = {K}: the faithful loop's loading backward error {worst_bw:.3e} (bar {SELF_BW:.0e})"


def test_flat_cases_cover_the_pivot_pairing_classes():
    assert set(kp.WIDE) <= set(kp.FLAT_CASES) and set(kp.FLAT_MODE_CASES) <= set(kp.CASES)
    narrow = kp.members("lambda", kp.K_MIN, 32)
    for ke, Ks in narrow.items():
        if ke >= 16:                     # k_lambda<8> is tests/test_gpu_parity.py's; from KE 16 on pivots pair
            assert set(Ks) & set(kp.FLAT_CASES), f"k_lambda<{ke}>: no flat-start case"
    assert (kp.FLAT_BURNIN, kp.FLAT_MCMC, kp.FLAT_THIN) == (0, 1, 1)
    st, flat = kp.case(23)["st"], kp.flat_start(23)
    assert np.all(flat.delta == 1.0) and np.all(flat.tauh == 1.0) and np.array_equal(flat.Plam, flat.psi)
    assert np.any(st.tauh != 1.0), "flat_start changed the shared case"
    for f in ("Lambda", "ps", "omega", "psi", "X", "Z", "eta"):
        assert np.array_equal(getattr(flat, f), getattr(st, f))


@pytest.mark.parametrize("K", kp.FLAT_ALL, ids=kp.case_id)
def test_flat_reference_is_well_posed(K):
    from helpers import rel_err, stagewise_errors
    from oracle import vectorised as V
    c = kp.flat_case(K)
    dr = c["src"].iteration(1)
    ref = c["st"].copy()
    assert not np.any(ref.Lambda)
    F.gibbs_iteration(ref, c["Yd"], c["rho"], c["hyper"], dr)
    errs, bw, _, (sbw, cond) = stagewise_errors(c["st"], ref.as_dict(), c["Yd"], c["rho"], c["hyper"], dr, scaled=True)
    vec = V.gibbs_iteration(c["st"].copy(), c["Yd"], c["rho"], c["hyper"], dr)
    fwd = rel_err(ref.Lambda, vec.Lambda)
    D = V._as_data(c["Yd"])
    st = c["st"].copy()
    V.update_ZX(st, D, c["rho"], dr)
    V.update_eta(st, c["rho"])
    condQ = float(np.linalg.cond(V.loading_systems(st, D, dr)[2]).max())
    xmax = float(np.abs(ref.X).max())
    print("K_PATHS_FLAT_REFERENCE", kp.case_id(K), kp.shape(K), {f: f"{e:.2e}" for f, e in sorted(errs.items())},
          f"lambda_bw {bw:.2e} lambda_sbw {sbw.max():.2e} cond(DQD) {cond.max():.3g} cond(Q) {condQ:.3g} "
          f"Lambda forward {fwd:.2e} max|X| {xmax:.3g}")
    for f in ("ps", "omega"):
        v = getattr(ref, f)
        assert np.all(np.isfinite(v)) and np.all(v > 0.0), f"flat K = {K}: reference {f} out of range"
    for f, e in errs.items():
        assert e <= SELF_TOL, f"flat K = {K}: the oracle's two flavours differ in {f} by {e:.3e} (bar {SELF_TOL:.0e})"
    assert bw <= SELF_BW, f"flat K = {K}: the faithful loop's loading backward error {bw:.3e} (bar {SELF_BW:.0e})"
    assert fwd <= SELF_TOL, f"flat K = {K}: the two flavours' Lambda differ forward by {fwd:.3e} (bar {SELF_TOL:.0e})"
    assert condQ <= FLAT_COND, f"flat K = {K}: cond(Q_j) {condQ:.3g}: a forward bar on Lambda needs another n or seed"
    assert xmax <= FLAT_XMAX, f"flat K = {K}: max|X| {xmax:.3g}"
