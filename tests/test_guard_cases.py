"""The preconditions of tests/test_gpu_guard.py, checked on the reference alone (no GPU): the planted cases of
tests/guard_cases.py do what their construction says, and guard_ratio restates what it claims to.

  1. eta after an iteration from Lambda = 0 does not depend on Yd (bitwise): the construction may build Yd around it.
  2. At every iteration (the oracle's own state, from the case's start state) the rows planted for it and the zero
     columns classify 'reject' and no other row is 'grey' or 'reject'.  A shape that misses this gets another n
     or seed, not another band.
  3. The oracle's states stay finite, ps and omega positive (with 2. no row is 'grey' at the second iteration
     either, inside the 5 % the GPU test could live with).
  4. On a stationary make_case state guard_ratio's sums reproduce, to 1e-9 relative, a direct evaluation of the
     quantities they stand for (|w|^2 = lambda' Q lambda, w.v = ps lambda.C, the identity's SS = dc:169's
     residual), and its numerator bounds the magnitudes the identity sums.
"""
import numpy as np
import pytest

import guard_cases as gc
from helpers import make_case
from oracle import dc_oracle as F
from oracle import vectorised as V

GREY_MAX = 0.05
RESTATE_TOL = 1e-9


def _oracle_iterations(c, n_iter):
    """[(start, state after)] of the oracle's iterations 1 .. n_iter on the planted case, each from the case's
    start state (guard_cases: the chain is not continued), dc:169 by the residual itself."""
    out = []
    for it in range(1, n_iter + 1):
        st = c["st"].copy()
        V.gibbs_iteration(st, c["Yd"], c["rho"], c["hyper"], c["src"].iteration(it), direct=True)
        out.append((c["st"].copy(), st))
    return out


def test_eta_first_does_not_depend_on_the_data():
    c = make_case(40, 42, 2, 7, seed=gc.SEED)
    d = c["src"].iteration(1)
    other = np.random.default_rng(1).standard_normal(c["Yd"].shape) * 1e6
    a, b = gc.eta_first(c["st"], c["Yd"], c["rho"], d), gc.eta_first(c["st"], other, c["rho"], d)
    assert np.array_equal(a, b)
    p = gc.planted_case("narrowA")
    assert np.array_equal(gc.eta_first(p["st"], p["Yd"], p["rho"], p["src"].iteration(1)), p["eta"][1])


@pytest.mark.parametrize("name", list(gc.CASES))
def test_planted_rows_and_no_others_reject(name):
    c = gc.planted_case(name)
    spec = gc.CASES[name]
    P, g = spec["shape"][1], spec["shape"][2]
    chain = _oracle_iterations(c, spec["n_iter"])
    assert sum(len(gc.planted_rows(name, it)) for it in range(1, spec["n_iter"] + 1)) == \
        len(spec["plants"]) + spec["n_iter"] * len(spec["zero_cols"])
    for it, (start, st) in enumerate(chain, start=1):
        planted = np.zeros((g, P), dtype=bool)
        for m, j in gc.planted_rows(name, it):
            planted[m, j] = True
        for f in ("ps", "omega", "Lambda", "eta"):
            v = getattr(st, f)
            assert np.all(np.isfinite(v)), f"{name} iteration {it}: reference {f} not finite"
        assert np.all(st.ps > 0.0) and np.all(st.omega > 0.0), f"{name} iteration {it}: reference ps / omega <= 0"
        ratio = gc.guard_ratio(start, st.as_dict(), c["Yd"], c["src"].iteration(it), gc.is_wide(name))
        cls = gc.classify(ratio)
        s = gc.summary(ratio, cls)
        SS = V.residual_ss(V.Data(c["Yd"]), st, np.ascontiguousarray(np.moveaxis(st.Lambda, 2, 0)))
        print(f"GUARD_CASES {name} iter {it}: {s}; dc:169 SS of the planted rows "
              f"{SS[planted].min():.3g} .. {SS[planted].max():.3g}")
        assert np.all(cls[planted] == "reject"), f"{name} iteration {it}: a planted row is not rejected: {ratio[planted]}"
        assert np.all(cls[~planted] == "accept"), \
            f"{name} iteration {it}: an unplanted row is not clear of the threshold: max ratio {ratio[~planted].max():.3g}"
        assert s["n_grey"] <= GREY_MAX * ratio.size
        # ps really depends on SS for the scaled rows: SS_j ~ n against bs = 0.3
        for m, j, _, t in spec["plants"]:
            assert SS[m, j] > 10.0 * c["hyper"].bs


@pytest.mark.parametrize("wide", [False, True], ids=["narrow_sums", "wide_sums"])
def test_guard_ratio_restates_what_it_bounds(wide):
    n, P, g, K = (40, 21, 2, 12) if not wide else (60, 37, 2, 40)
    c = make_case(n, P * g, g, K, seed=gc.SEED)
    st = c["st"].copy()
    for it in range(1, 4):                                   # a stationary state: Lambda, psi o tau are real
        F.gibbs_iteration(st, c["Yd"], c["rho"], c["hyper"], c["src"].iteration(it))
    start = st.copy()
    d = c["src"].iteration(4)
    V.gibbs_iteration(st, c["Yd"], c["rho"], c["hyper"], d, direct=True)
    p = gc.guard_parts(start, st.as_dict(), c["Yd"], d, wide)
    lam, Q, E, C, ps, yy = p["lam"], p["Q"], p["E"], p["C"], p["ps"], p["yy"]

    def rel(a, b):
        return float(np.max(np.abs(a - b) / np.abs(b)))

    lQl = np.einsum("mjk,mjkl,mjl->mj", lam, Q, lam)
    lEl = np.einsum("mjk,mkl,mjl->mj", lam, E, lam)
    SS = V.residual_ss(V.Data(c["Yd"]), st, lam)
    assert rel(p["ww"], lQl) < RESTATE_TOL                    # x'Q x = |w|^2
    assert rel(p["wv"], ps * p["lc"]) < RESTATE_TOL           # ps x.C = w.v
    assert rel((p["ww"] - p["px"]) / ps, lEl) < RESTATE_TOL   # x'E x
    assert rel(p["SS"], SS) < RESTATE_TOL                     # the identity against dc:169 as written
    # the numerator bounds the magnitudes the identity sums, by either of its two routes
    terms = yy + 2.0 * np.einsum("mjk,mjk->mj", np.abs(lam), np.abs(C)) + \
        np.einsum("mjk,mkl,mjl->mj", np.abs(lam), np.abs(E), np.abs(lam))
    assert np.all((1.01 * (np.sqrt(yy) + p["sabs"])) ** 2 >= terms)
    assert np.all(p["num"] >= yy + 2.0 * np.abs(p["lc"]) + lEl)
    ratio = gc.guard_ratio(start, st.as_dict(), c["Yd"], d, wide)
    assert np.array_equal(ratio, p["num"] / p["SS"]) and np.all(ratio >= 1.0)


def test_classify_band():
    r = np.array([0.0, 499.9, 500.0, 1000.0, 2000.0, 2000.1, np.inf, np.nan])
    assert list(gc.classify(r)) == ["accept", "accept", "grey", "grey", "grey", "reject", "reject", "grey"]


def test_zero_column_rejects_whatever_its_ratio():
    c = gc.planted_case("narrowA")
    (start, st), = _oracle_iterations(c, 1)
    p = gc.guard_parts(start, st.as_dict(), c["Yd"], c["src"].iteration(1), False)
    m, j = gc.CASES["narrowA"]["zero_cols"][0]
    assert p["yy"][m, j] == 0.0 and np.isfinite(p["SS"][m, j]) and p["SS"][m, j] > 0.0
    assert gc.guard_ratio(start, st.as_dict(), c["Yd"], c["src"].iteration(1), False)[m, j] == np.inf
