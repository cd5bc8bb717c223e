"""The decision of the SS identity's guard (csrc/resid.h, ss_identity_reject) and both of its fallbacks, on the
planted cases of tests/guard_cases.py (the construction, the case table and why a two-iteration case sets its start
state again; tests/test_guard_cases.py checks the cases on the reference, on the CPU).

Everywhere else in the suite the guard either rejects every row (DCFM_FLAG_GUARD_ALL) or, at the small shapes, none.
Here chosen rows reject (kappa_j = 1e5 ... 1e17 against the threshold 1e3; a zero column) while their neighbours
accept, so the decision, the row it is taken for and the mixing of the two paths in one launch are exercised:
K <= 32 the wave's 8 rows through resid_rows8 inside k_lambda, K > 32 the row's 32-row tile through rflag and
k_resid_flagged (PP / 32 = 18 tiles over 16 blocks in case wideF, so a block walks two tiles).

Injected draws, one iteration per run call, every iteration saved; each case in the default mode and in
DCFM_FLAG_GUARD_ALL.  After every iteration, no row left out:
  * ps and omega per row, unscaled relative, against oracle.dc_oracle.update_ps (dc:169 as written) on the device's
    own eta and Lambda, within max(1e-10, helpers.residual_rounding_bound); the bound exceeds 1e-10 on rows that
    classify 'reject' only;
  * the decision, rejected side: a wave (K <= 32) or 32-row tile (K > 32) that holds a 'reject' row has ps and omega
    bitwise equal to the GUARD_ALL run in all of its valid rows (both runs have bitwise the same eta and Lambda:
    asserted);
  * the decision, accepted side: over the waves or tiles whose rows all classify 'accept', at least one row differs
    in bits from GUARD_ALL (an identity SS and a residual SS agree to rounding, not in bits); in case wideF the same
    within every block's pair of tiles (t, t + 16), which is what shows a flag of the iteration before that was not
    cleared: the tiles flagged at iteration 1 are all 'accept' at iteration 2;
  * X, Z, eta within 1e-10 of the oracle's and the loading draw's backward error <= 1e-13
    (helpers.stagewise_errors): every iteration starts from the case's start state, Lambda = 0.
After the run saved_samples() is the number of iterations, Sigmaout is exactly symmetric and within 1e-12 normwise
of the host's mean of oracle.dc_oracle.assemble_sample over the device's own saved states (a wave that added its
omega to wsum before and after switching to the residual would double it: 1e-7 of case narrowC's Sigmaout).

Measured on the MI355X: DESIGN.md section 2, "The guard's decision", with the outcome of raising
KAPPA_IDENTITY_MAX to 1e30.
"""
import functools

import numpy as np
import pytest

import guard_cases as gc
from helpers import as_oracle_state, residual_rounding_bound, scaled_rel_err, stacked_draws, stagewise_errors, state_dict
from oracle import dc_oracle as F

pytestmark = pytest.mark.gpu

TOL = 1e-10           # the project's bar (ps, omega per row; X, Z, eta normwise)
BW_TOL = 1e-13        # loading backward error
SIGMA_TOL = 1e-12     # Sigmaout against the host sum of the device's own samples
GUARD_ALL = 0x40      # include/dcfm.h
MODES = {"default": 0, "guard_all": GUARD_ALL}


@functools.lru_cache(maxsize=None)
def _run(dcfm, name, mode):
    """Case `name` in `mode`: the state after each iteration (each from the start state, set again on the same
    handle), Sigmaout and the saved-sample count.  Made once, shared, read only."""
    c = gc.planted_case(name)
    n, P, g, K = gc.CASES[name]["shape"]
    n_iter = gc.CASES[name]["n_iter"]
    start = {f: v for f, v in state_dict(c["st"]).items() if f != "eta"}
    smp = dcfm.Sampler(n, P, g, K, c["rho"], 0, n_iter, 1, inject_draws=True, flags=MODES[mode])
    try:
        smp.set_data(c["Yd"])
        smp.set_draws(stacked_draws(c["src"], 1, n_iter), 1, n_iter)
        states = []
        for it in range(1, n_iter + 1):
            smp.set_state(start)
            smp.run(it, 1)
            states.append(smp.get_state())
        out = dict(states=states, sigma=smp.get_sigma(), saved=smp.saved_samples())
    finally:
        smp.close()
    for st in out["states"]:
        for v in st.values():
            v.setflags(write=False)
    out["sigma"].setflags(write=False)
    return out


def _rows(a, P, g):
    """ps (P x 1 x g) or omega (P x g) as g x P."""
    return np.asarray(a, dtype=np.float64).reshape(P, g).T


def _groups(name, cls):
    """[(m, first row, last row + 1, 'reject' | 'accept' | 'mixed')] of every wave (K <= 32) or 32-row tile (K > 32):
    'reject' if a row of it classifies so, 'accept' if all do, 'mixed' if a row is grey and none rejects."""
    g, P = cls.shape
    R = gc.group_rows(name)
    out = []
    for m in range(g):
        for r0 in range(0, P, R):
            k = cls[m, r0:min(r0 + R, P)]
            out.append((m, r0, min(r0 + R, P), "reject" if np.any(k == "reject") else
                        "accept" if np.all(k == "accept") else "mixed"))
    return out


def _check_accuracy(name, it, got, cls, worst):
    c = gc.planted_case(name)
    errs, bw, _, (sbw, cond) = stagewise_errors(c["st"], got, c["Yd"], c["rho"], c["hyper"], c["src"].iteration(it),
                                                scaled=True)
    ref = c["st"].copy()
    for f in ("eta", "Lambda"):
        getattr(ref, f)[...] = np.asarray(got[f], dtype=np.float64).reshape(getattr(ref, f).shape)
    F.update_ps(ref, c["Yd"], c["hyper"], c["src"].iteration(it))            # dc:169-171 as written
    bound = residual_rounding_bound(got, c["Yd"])                             # g x P
    e = {f: scaled_rel_err(got[f], getattr(ref, f), bound.T, TOL) for f in ("ps", "omega")}
    loose = bound > TOL
    # the diagonally scaled loading measure beside the normwise one: printed and recorded, not asserted (the
    # planted start, Plam_j = 1e-12, has not been measured against the reference: tests/test_loading_measure.py)
    worst.update(ps=e["ps"], omega=e["omega"], X=errs["X"], Z=errs["Z"], eta=errs["eta"], lambda_bw=bw,
                 lambda_sbw=float(sbw.max()), cond_dqd=float(cond.max()),
                 bound_max=float(bound.max()), bound_max_not_rejected=float(bound[cls != "reject"].max()))
    return e, errs, bw, loose


def _check(dcfm, name, mode, record_property):
    c = gc.planted_case(name)
    n, P, g, K = gc.CASES[name]["shape"]
    n_iter = gc.CASES[name]["n_iter"]
    r, ga = _run(dcfm, name, mode), _run(dcfm, name, "guard_all")
    assert len(r["states"]) == n_iter
    for it in range(1, n_iter + 1):
        got, all_ = r["states"][it - 1], ga["states"][it - 1]
        ratio = gc.guard_ratio(c["st"], got, c["Yd"], c["src"].iteration(it), gc.is_wide(name))
        cls = gc.classify(ratio)
        worst = gc.summary(ratio, cls)
        e, errs, bw, loose = _check_accuracy(name, it, got, cls, worst)
        # the decision: which waves / tiles carry the residual's bits
        groups = _groups(name, cls)
        same = {f: _rows(got[f], P, g) == _rows(all_[f], P, g) for f in ("ps", "omega")}
        differing = {(m, r0): int(np.sum(~(same["ps"][m, r0:r1] & same["omega"][m, r0:r1])))
                     for m, r0, r1, _ in groups}
        worst.update(groups_reject=sum(k == "reject" for *_, k in groups),
                     groups_accept=sum(k == "accept" for *_, k in groups),
                     accept_rows_differing=sum(differing[m, r0] for m, r0, _, k in groups if k == "accept"))
        print(f"GUARD {name} {mode} iter {it}:", {f: (f"{v:.3e}" if isinstance(v, float) else v) for f, v in worst.items()})
        for f, v in worst.items():
            record_property(f"it{it}_{f}", v)
        for f in ("ps", "omega"):
            assert e[f] < TOL, f"{name} {mode} iteration {it}: {f} vs dc:169 on the device's own state {e[f]:.3e} (bar {TOL:.0e})"
        assert np.all(cls[loose] == "reject"), \
            f"{name} {mode} iteration {it}: the rounding bound exceeds {TOL:.0e} on a row that is not rejected"
        for f in ("X", "Z", "eta"):
            assert errs[f] < TOL, f"{name} {mode} iteration {it}: stage {f} rel err {errs[f]:.3e} (bar {TOL:.0e})"
        assert bw <= BW_TOL, f"{name} {mode} iteration {it}: loading backward error {bw:.3e} (bar {BW_TOL:.0e})"
        planted = gc.planted_rows(name, it)
        assert all(cls[m, j] == "reject" for m, j in planted), f"{name} iteration {it}: a planted row does not classify 'reject'"
        if mode != "default":
            continue
        for f in ("eta", "Lambda"):
            assert np.array_equal(got[f], all_[f]), f"{name} iteration {it}: {f} differs between the two modes"
        for m, r0, r1, kind in groups:
            if kind == "reject":
                assert differing[m, r0] == 0, \
                    (f"{name} iteration {it}: shard {m} rows {r0}..{r1 - 1} hold a rejected row, but {differing[m, r0]} "
                     f"of them do not carry the residual's ps / omega (ratios {ratio[m, r0:r1]})")
        accepted = [(m, r0) for m, r0, _, k in groups if k == "accept"]
        assert accepted and sum(differing[x] for x in accepted) > 0, \
            f"{name} iteration {it}: every accepted wave / tile carries the residual's bits: the guard rejects too much"
        if name == "wideF":          # k_resid_flagged's blocks: block b walks tiles b and b + 16
            for b in range(gc.WIDE_BLOCKS):
                pair = [(0, 32 * t) for t in (b, b + gc.WIDE_BLOCKS) if (0, 32 * t) in accepted]
                assert not pair or sum(differing[x] for x in pair) > 0, \
                    f"wideF iteration {it}: block {b}'s accepted tiles {pair} carry the residual's bits (a stale flag?)"
    # the saved samples
    S = r["sigma"]
    assert r["saved"] == n_iter
    assert np.all(np.isfinite(S)) and np.array_equal(S, S.T), "Sigmaout not exactly symmetric"
    want = sum(F.assemble_sample(as_oracle_state(st), c["rho"]) for st in r["states"]) / n_iter
    serr = float(np.max(np.abs(S - want)) / np.max(np.abs(want)))
    print(f"GUARD {name} {mode} Sigmaout vs the device's own samples: {serr:.3e}")
    record_property("sigma", serr)
    assert serr < SIGMA_TOL, f"{name} {mode}: Sigmaout vs the device's own samples {serr:.3e} (bar {SIGMA_TOL:.0e})"


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(gc.CASES))
def test_planted_rows(dcfm, name, mode, record_property):
    _check(dcfm, name, mode, record_property)
