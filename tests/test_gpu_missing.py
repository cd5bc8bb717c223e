"""Missing training data on the device (dcfm_set_missing / dcfm_get_imputed, csrc/impute.hip).

  1. the step is the conditional: after every stepped call the observed entries of Y are the input bit for bit and
     every missing one is eta_i . lambda_j + z / sqrt(ps_j) of the device's own state, z from the host restatement
     of the Philox stream at site 13;
  2. the sweep reads the completed data: iteration t passes the stage-wise checks against the oracle on Y_{t-1}, the
     completed matrix read before the call (ps / omega per row are what a stale yy breaks);
  3. replay: one call, one iteration per call and a ragged split give the same bits, as do two loopback ranks and
     a COMM_SELF handle;
  4. the accumulators against host sums of the stepped mu and 1 / ps;
  5. off means off;  6. continuation from get_data;  7. errors;  8. coexistence with every other per-sample feature;
  9. it imputes: 8 chains against the reference chains of tests/golden/missing_chain.json, through the Sampler and
     through divideconquer(..., impute=True).

The sweep's draws are injected (helpers.make_case / stacked_draws); the step's normals always come from Philox at
the handle's seed.

Bars.  Test 1: 1e-12 (sum_k |eta_ik lambda_jk| + |z| / sqrt(ps_j)), derived: a K <= 128 dot product is within
(K + 2) 2^-53 of that magnitude sum and the normals within the 2 F_n bar of test_gpu_rng_exact.py, about 50 x
margin.  Test 2: the project's 1e-10 stage-wise and 1e-13 loading backward error.  Test 4: 1e-12 relative.
Measured on the MI355X, worst ratio to the bar: test 1 4.1e-4, test 2 5.3e-4 (stages) and 1.9e-3 (backward error),
test 4 4.0e-4; test 9 r 0.762 - 0.779 and c 0.977 - 0.981 against the reference's 0.761 - 0.765 and 0.978 - 0.981.
"""
import json
import threading
from pathlib import Path

import numpy as np
import pytest

import missing_cases as mc
from helpers import as_oracle_state as _as_oracle, make_case, rel_err, stacked_draws, stagewise_errors, state_dict

pytestmark = pytest.mark.gpu

STEP_BAR = 1e-12
TOL, BW_TOL = 1e-10, 1e-13
ACC_BAR = 1e-12
NSTEP = 4
# replay: 9 iterations, burn-in 3, thin 2 (saved 4, 6, 8), assembly batches of 2
RN, RBURN, RTHIN, RBATCH = 9, 3, 2, 2
R_ONE = [(1, 9)]
R_STEPPED = [(t, 1) for t in range(1, RN + 1)]
R_RAGGED = [(1, 2), (3, 1), (4, 0), (4, 4), (8, 2)]
SHAPES = dict(mc.CASES, R4=((37, 44, 4, 3), 0), R4U=((37, 44, 4, 3), mc.UNFUSED))       # g = 4: the rank tests only

_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _case(name):
    def build():
        (n, p, g, K), _ = SHAPES[name]
        c = make_case(n, p, g, K, seed=mc.CASE_SEED)
        c["Yd"].setflags(write=False)
        c["draws"] = stacked_draws(c["src"], 1, RN)
        c["init"] = {f: v for f, v in state_dict(c["st"]).items() if f != "eta"}
        return c
    return _once(("case", name), build)


def _mask(name, pattern):
    c = _case(name)
    return mc.make_mask(pattern, c["n"], c["P"], c["g"])


def _local(c, s0, gl):
    return {f: (v if f in ("X", "delta", "tauh") else v[..., s0:s0 + gl]) for f, v in c["init"].items()}


def _open(dcfm, name, mask, *, flags=0, burnin=0, mcmc=RN, thin=1, asm_batch=0, capacity=None, Yd=None, state=None,
          nranks=1, rank=0, comm=True, **kw):
    """A handle of the case with data, mask, state and injected draws set."""
    c = _case(name)
    gl = c["g"] // nranks
    s0 = rank * gl
    smp = dcfm.Sampler(c["n"], c["P"], c["g"], c["K"], c["rho"], burnin, mcmc, thin, seed=mc.CHAIN_SEED,
                       inject_draws=True, flags=SHAPES[name][1] | flags, asm_batch=asm_batch, nranks=nranks, rank=rank,
                       **kw)
    try:
        if comm and (flags & mc.COMM_SELF):
            smp.comm_init(dcfm.Sampler.unique_id())
        smp.set_data((c["Yd"] if Yd is None else Yd)[:, :, s0:s0 + gl])
        if mask is not None:
            smp.set_missing(mask[:, :, s0:s0 + gl], capacity)
        smp.set_state(_local(c, s0, gl) if state is None else state)
        smp.set_draws(c["draws"], 1, RN)
    except Exception:
        smp.close()
        raise
    return smp


def _stepped(dcfm, name, pattern, flags=0, mask=None):
    """NSTEP iterations, one per call: [(Y before, state before, state after, Y after)] per iteration (`mask`: the
    mask itself where `pattern` is not one of missing_cases.make_mask's)."""
    def run():
        mk = _mask(name, pattern) if mask is None else mask
        smp = _open(dcfm, name, mk, flags=flags, capacity=0)
        out = []
        try:
            Y, st = smp.get_data(), smp.get_state()
            for it in range(1, NSTEP + 1):
                smp.run(it, 1)
                st2, Y2 = smp.get_state(), smp.get_data()
                out.append((Y, st, st2, Y2))
                Y, st = Y2, st2
        finally:
            smp.close()
        return out
    return _once(("stepped", name, pattern, flags), run)


# ---- 1 ---------------------------------------------------------------------------------------------
STEP_CASES = [("A", p) for p in mc.PATTERNS] + [(n, p) for n in "BCD" for p in ("random", "edges")]


def _check_step(c, mask, steps, what):
    """The step is the conditional: `steps` is _stepped's list for the case c under `mask`."""
    worst = 0.0
    for it, (Y0, _, got, Y1) in enumerate(steps, start=1):
        assert np.array_equal(Y1[~mask], c["Yd"][~mask]), f"iteration {it}: an observed entry moved"
        if not mask.any():
            continue
        z = mc.impute_normals(mc.CHAIN_SEED, c["n"], c["P"], range(c["g"]), it)
        want, _ = mc.impute_ref(Y0, mask, got["eta"], got["Lambda"], got["ps"], z)
        mag = mc.magnitude(mask, got["eta"], got["Lambda"], got["ps"], z)
        ratio = float(np.max(np.abs(Y1 - want)[mask] / (STEP_BAR * mag[mask])))
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"iteration {it}: a missing entry is off its conditional draw by {ratio:.3g} x the bar"
        assert not np.array_equal(Y1[mask], Y0[mask])                       # the entries were redrawn
    print(f"MISSING_STEP {what}: worst ratio to the 1e-12 bar {worst:.3e}")
    return worst


@pytest.mark.parametrize("name,pattern", STEP_CASES)
def test_the_step_is_the_conditional(dcfm, name, pattern):
    _check_step(_case(name), _mask(name, pattern), _stepped(dcfm, name, pattern), f"{name} {pattern}")


# ---- 2 ---------------------------------------------------------------------------------------------
def _check_sweep(c, steps, what):
    """The sweep reads the completed data: iteration t of `steps` (_stepped's list) against the oracle on Y_{t-1}."""
    worst, worst_bw = {}, 0.0
    for it, (Y0, st0, got, _) in enumerate(steps, start=1):
        errs, bw, _, (sbw, cond) = stagewise_errors(_as_oracle(st0), got, Y0, c["rho"], c["hyper"],
                                                    c["src"].iteration(it), scaled=True)
        for f, e in errs.items():
            worst[f] = max(worst.get(f, 0.0), e)
        worst_bw = max(worst_bw, bw)
        # the scaled loading measure is printed beside the normwise one, not asserted (these states have not been
        # measured against the reference: tests/test_loading_measure.py)
        print(f"MISSING_STAGEWISE {what} it {it}:", {k: f"{v:.2e}" for k, v in errs.items()},
              f"bw {bw:.2e} sbw {sbw.max():.2e} cond(DQD) <= {cond.max():.2e}")
        for f, e in errs.items():
            assert e < TOL, f"iteration {it}: stage {f} rel err {e:.3e} (bar {TOL:.0e})"
        assert bw <= BW_TOL, f"iteration {it}: loading backward error {bw:.3e} (bar {BW_TOL:.0e})"
    print(f"MISSING_STAGEWISE_WORST {what}: stage {max(worst.values()) / TOL:.3e} x bar,"
          f" bw {worst_bw / BW_TOL:.3e} x bar")
    return max(worst.values()), worst_bw


@pytest.mark.parametrize("flags", [0, mc.EXACT_RESIDUAL, mc.GUARD_ALL], ids=["default", "exact", "guard_all"])
@pytest.mark.parametrize("name", ["A", "C"])
def test_the_sweep_reads_the_completed_data(dcfm, name, flags):
    _check_sweep(_case(name), _stepped(dcfm, name, "random", flags), f"{name} flags {flags:#x}")


def test_yy_is_rewritten_not_incremented(dcfm):
    """What a stale yy does: the same iteration with Y_{t-1}'s missing entries replaced in the oracle's data by the
    values of Y_{t-2} misses the ps bar by orders of magnitude -- the check of test 2 can tell."""
    c = _case("A")
    steps = _stepped(dcfm, "A", "random")
    (Yold, _, _, _), (Y0, st0, got, _) = steps[0], steps[1]
    errs, _, _ = stagewise_errors(_as_oracle(st0), got, Yold, c["rho"], c["hyper"], c["src"].iteration(2))
    assert errs["ps"] > 1e3 * TOL


# ---- 3 ---------------------------------------------------------------------------------------------
def _read(smp):
    mean, m2, nvar, cnt = smp.imputed_raw()
    return {"state": smp.get_state(), "Y": smp.get_data(), "mean": mean, "m2": m2, "nvar": nvar, "count": cnt,
            "saved": smp.saved_samples()}


def _run_plan(dcfm, name, mask, plan, **kw):
    smp = _open(dcfm, name, mask, burnin=RBURN, mcmc=RN - RBURN, thin=RTHIN, asm_batch=RBATCH, **kw)
    try:
        for first, n in plan:
            smp.run(first, n)
        out = _read(smp)
        out["sigma"] = smp.get_sigma()
    finally:
        smp.close()
    return out


def _assert_same(a, b, what, fields=("Y", "mean", "m2", "nvar")):
    for f in a["state"]:
        assert np.array_equal(a["state"][f], b["state"][f]), f"{what}: state {f} not bitwise equal"
    for f in fields:
        assert np.array_equal(a[f], b[f]), f"{what}: {f} not bitwise equal"
    assert a["count"] == b["count"] and a["saved"] == b["saved"], what


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_replay(dcfm, name):
    mask = _mask(name, "random")
    one = _once(("replay_one", name), lambda: _run_plan(dcfm, name, mask, R_ONE))
    assert one["count"] == one["saved"] == 3 and np.all(np.isfinite(one["mean"])) and np.all(np.isfinite(one["nvar"]))
    assert not np.array_equal(one["Y"][mask], _case(name)["Yd"][mask])
    for plan, what in ((R_STEPPED, "one iteration per call"), (R_RAGGED, "ragged split"), (R_ONE, "a fresh handle")):
        _assert_same(_run_plan(dcfm, name, mask, plan), one, f"{name} {what} vs one call")


def _run_ranks(dcfm, name, mask, plan, nranks):
    c = _case(name)
    gl = c["g"] // nranks
    smps = [dcfm.Sampler(c["n"], c["P"], c["g"], c["K"], c["rho"], RBURN, RN - RBURN, RTHIN, seed=mc.CHAIN_SEED,
                         inject_draws=True, flags=SHAPES[name][1], asm_batch=RBATCH, nranks=nranks, rank=r)
            for r in range(nranks)]
    try:
        dcfm.Sampler.comm_loopback(smps)
        for r, smp in enumerate(smps):
            smp.set_data(c["Yd"][:, :, r * gl:(r + 1) * gl])
            smp.set_missing(mask[:, :, r * gl:(r + 1) * gl])
            smp.set_state(_local(c, r * gl, gl))
            smp.set_draws(c["draws"], 1, RN)
        out, errs = [None] * nranks, []

        def work(r):
            try:
                for first, n in plan:
                    smps[r].run(first, n)
                out[r] = _read(smps[r])
            except Exception as e:                           # surfaced below
                errs.append(e)

        ths = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=100)
        assert not any(t.is_alive() for t in ths), "a rank did not finish"
        assert not errs, errs
        return out
    finally:
        for smp in smps:
            smp.close()


@pytest.mark.parametrize("name", ["R4", "R4U"])
def test_ranks_replay(dcfm, name):
    c = _case(name)
    mask = _mask(name, "random")
    one = _run_plan(dcfm, name, mask, R_ONE)
    assert one["count"] == 3
    ranks = _run_ranks(dcfm, name, mask, R_ONE, 2)
    gl = c["g"] // 2
    for r, got in enumerate(ranks):
        sl = slice(r * gl, (r + 1) * gl)
        for f, v in got["state"].items():
            want = one["state"][f] if f in ("X", "delta", "tauh") else one["state"][f][..., sl]
            assert np.array_equal(v, want), f"rank {r}: state {f} is not the one-rank chain's"
        for f in ("Y", "mean", "m2", "nvar"):
            assert np.array_equal(got[f], one[f][..., sl]), f"rank {r}: {f} is not the one-rank chain's slice"
        assert got["count"] == 3
    own = _run_plan(dcfm, name, mask, R_ONE, flags=mc.COMM_SELF)
    _assert_same(own, one, f"{name} COMM_SELF vs the plain handle")


# ---- 4 ---------------------------------------------------------------------------------------------
def _accumulate(dcfm, name, mask, capacity, second_call_at=None):
    """Stepped run of the replay shape; returns the read-out and the host sums over the accumulated iterations."""
    c = _case(name)
    smp = _open(dcfm, name, mask, burnin=RBURN, mcmc=RN - RBURN, thin=RTHIN, asm_batch=RBATCH, capacity=capacity)
    s1, s2, sv, cnt = np.zeros(mask.shape), np.zeros(mask.shape), np.zeros(mask.shape[1:]), 0
    try:
        y_start = smp.get_data()
        for it in range(1, RN + 1):
            if it == second_call_at:
                smp.set_missing(mask, capacity)
                s1[...], s2[...], sv[...], cnt = 0.0, 0.0, 0.0, 0
            smp.run(it, 1)
            if it % RTHIN == 0 and it > RBURN and cnt < capacity:
                st = smp.get_state(("eta", "Lambda", "ps"))
                mu = np.einsum("ikm,jkm->ijm", st["eta"], st["Lambda"])
                s1 += mu
                s2 += mu * mu
                sv += 1.0 / st["ps"][:, 0, :]
                cnt += 1
        out = _read(smp)
    finally:
        smp.close()
    return out, s1, s2, sv, cnt, y_start


def _check_accumulators(dcfm, name, mask):
    """get_imputed's accumulators against host sums of the stepped mu and 1 / ps."""
    has = mask.any(axis=0)
    worst = 0.0
    for capacity, second in ((3, None), (2, None), (3, 5)):
        got, s1, s2, sv, cnt, _ = _accumulate(dcfm, name, mask, capacity, second)
        assert got["count"] == cnt == (2 if capacity == 2 or second else 3) and got["saved"] == 3
        for f, want in (("mean", s1 / cnt), ("m2", s2 / cnt)):
            # normwise over the missing entries (helpers.rel_err, the project's relative error): mu is a K-term dot
            # product of mixed sign, so an entry's own value is no scale for its rounding error
            e = rel_err(got[f][mask], want[mask])
            worst = max(worst, e)
            assert e <= ACC_BAR, f"{f}: {e:.3e}"
        e = np.abs(got["nvar"] - sv / cnt)[has] / (sv / cnt)[has]
        worst = max(worst, float(e.max()))
        assert e.max() <= ACC_BAR and not got["nvar"][~has].any()
        assert np.array_equal(got["mean"][~mask], got["Y"][~mask]) and np.array_equal(got["m2"][~mask], got["Y"][~mask] ** 2)
    print(f"MISSING_ACC {name}: worst ratio to the 1e-12 bar {worst / ACC_BAR:.3e}")
    return worst / ACC_BAR


@pytest.mark.parametrize("name", ["A", "C"])
def test_accumulators(dcfm, name):
    _check_accumulators(dcfm, name, _mask(name, "edges"))


def test_capacity_zero_moves_the_chain_and_counts_nothing(dcfm):
    mask = _mask("A", "random")
    got, *_ , y_start = _accumulate(dcfm, "A", mask, 0)
    assert got["count"] == 0 and got["saved"] == 3
    assert not got["mean"].any() and not got["m2"].any() and not got["nvar"].any()       # nothing is written
    assert not np.array_equal(got["Y"][mask], y_start[mask]) and np.array_equal(got["Y"][~mask], y_start[~mask])
    with_acc = _once(("replay_one", "A"), lambda: _run_plan(dcfm, "A", mask, R_ONE))
    assert np.array_equal(got["Y"], with_acc["Y"])                                      # the accumulators move nothing
    smp = _open(dcfm, "A", mask, capacity=0)
    try:
        sm = smp.imputed()
        assert sm["count"] == 0 and np.array_equal(sm["mask"], mask) and not sm["sd_total"].any()
    finally:
        smp.close()


# ---- 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "C"])
def test_off_means_off(dcfm, name):
    def run(how):
        smp = _open(dcfm, name, _mask(name, "none") if how == "none" else None, burnin=RBURN, mcmc=RN - RBURN,
                    thin=RTHIN, asm_batch=RBATCH)
        try:
            if how == "cleared":
                smp.set_missing(_mask(name, "random"))
                smp.set_missing(None)
            smp.set_profiling(True)
            smp.run(1, RN)
            return {"state": smp.get_state(), "sigma": smp.get_sigma(), "Y": smp.get_data(),
                    "stats": {k: v[1] for k, v in smp.kernel_stats().items()}, "count": smp.imputed()["count"]}
        finally:
            smp.close()
    never, none, cleared = run("never"), run("none"), run("cleared")
    for other, what in ((none, "the none mask"), (cleared, "a cleared mask")):
        for f in never["state"]:
            assert np.array_equal(other["state"][f], never["state"][f]), f"{what}: state {f}"
        assert np.array_equal(other["sigma"], never["sigma"]) and np.array_equal(other["Y"], never["Y"]), what
        assert other["stats"] == never["stats"] and other["count"] == 0, what
    assert np.array_equal(never["Y"], _case(name)["Yd"])
    # and on: the same launches but one k_save scope per iteration more
    smp = _open(dcfm, name, _mask(name, "random"), burnin=RBURN, mcmc=RN - RBURN, thin=RTHIN, asm_batch=RBATCH)
    try:
        smp.set_profiling(True)
        smp.run(1, RN)
        on = {k: v[1] for k, v in smp.kernel_stats().items()}
    finally:
        smp.close()
    assert on["k_save"] == never["stats"]["k_save"] + RN
    assert {k: v for k, v in on.items() if k != "k_save"} == {k: v for k, v in never["stats"].items() if k != "k_save"}


# ---- 6 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "C"])
def test_continuation(dcfm, name):
    mask = _mask(name, "random")
    whole = _run_plan(dcfm, name, mask, [(1, 6)], capacity=0)
    smp = _open(dcfm, name, mask, burnin=RBURN, mcmc=RN - RBURN, thin=RTHIN, asm_batch=RBATCH, capacity=0)
    try:
        smp.run(1, 3)
        Y3, st3 = smp.get_data(), smp.get_state()
    finally:
        smp.close()
    rest = _run_plan(dcfm, name, mask, [(4, 3)], capacity=0, Yd=Y3, state={f: v for f, v in st3.items() if f != "eta"})
    for f in whole["state"]:
        assert np.array_equal(rest["state"][f], whole["state"][f]), f"continued chain: state {f} not bitwise equal"
    assert np.array_equal(rest["Y"], whole["Y"])


@pytest.mark.parametrize("name", ["A", "C"])
def test_nan_entries_start_from_zero(dcfm, name):
    c = _case(name)
    mask = _mask(name, "random")
    smp = _open(dcfm, name, mask, Yd=np.where(mask, np.nan, c["Yd"]), capacity=0)
    try:
        Y0, st0 = smp.get_data(), smp.get_state()
        assert not Y0[mask].any() and np.array_equal(Y0[~mask], c["Yd"][~mask])
        smp.run(1, 1)
        got, Y1 = smp.get_state(), smp.get_data()
    finally:
        smp.close()
    errs, bw, _ = stagewise_errors(_as_oracle(st0), got, Y0, c["rho"], c["hyper"], c["src"].iteration(1))
    for f, e in errs.items():
        assert e < TOL, f"stage {f} rel err {e:.3e}"
    assert bw <= BW_TOL and np.all(np.isfinite(Y1))


# ---- 7 ---------------------------------------------------------------------------------------------
def test_errors(dcfm):
    from dcfm_amd import _abi
    c = _case("A")
    mask = _mask("A", "random")
    smp = dcfm.Sampler(c["n"], c["P"], c["g"], c["K"], c["rho"], 0, NSTEP, 1, seed=mc.CHAIN_SEED, inject_draws=True)
    try:
        with pytest.raises(_abi.DcfmError) as ei:                           # the mask before the data
            smp.set_missing(mask)
        assert ei.value.code == _abi.DCFM_ERR_INVALID and "set_data first" in str(ei.value)
        smp.set_data(c["Yd"])
        smp.set_state(c["init"])
        smp.set_draws(c["draws"], 1, RN)
        with pytest.raises(_abi.DcfmError) as ei:
            smp.set_missing(mask, -1)
        assert ei.value.code == _abi.DCFM_ERR_INVALID
        assert smp.imputed()["count"] == 0
        # the mask first, then the log-likelihood: refused, the mask stays and works
        smp.set_missing(mask)
        with pytest.raises(_abi.DcfmError) as ei:
            smp.set_loglik(2)
        assert ei.value.code == _abi.DCFM_ERR_UNSUPPORTED
        smp.run(1, 2)
        assert smp.imputed()["count"] == 2 and smp.loglik_draws().shape[0] == 0
        assert not np.array_equal(smp.get_data()[mask], c["Yd"][mask])
        # set_data clears the mask
        smp.set_data(c["Yd"])
        smp.run(3, 1)
        assert np.array_equal(smp.get_data(), c["Yd"]) and smp.imputed()["count"] == 0
        # the log-likelihood first, then the mask: refused, the log-likelihood stays and works
        smp.set_loglik(2)
        with pytest.raises(_abi.DcfmError) as ei:
            smp.set_missing(mask)
        assert ei.value.code == _abi.DCFM_ERR_UNSUPPORTED
        smp.set_missing(None)                                              # turning it off is always allowed
        smp.run(4, 1)
        assert smp.loglik_draws().shape[0] == 1 and np.array_equal(smp.get_data(), c["Yd"])
    finally:
        smp.close()


def test_read_out_after_a_nan_state(dcfm):
    from dcfm_amd import _abi
    c = _case("A")
    mask = _mask("A", "random")
    smp = _open(dcfm, "A", mask, mcmc=NSTEP)
    try:
        smp.run(1, 1)
        bad = {f: np.array(v, copy=True) for f, v in c["init"].items()}
        bad["ps"][3, 0, 1] = np.nan
        smp.set_state(bad)
        smp.run(2, 1)
        with pytest.raises(_abi.DcfmError) as ei:
            smp.synchronize()
        assert ei.value.code == _abi.DCFM_ERR_NUMERIC
        mean, m2, nvar, cnt = smp.imputed_raw()                            # returns what the device holds
        assert cnt == 2 and mean.shape == mask.shape
        assert smp.get_data().shape == mask.shape
    finally:
        smp.close()


# ---- 8 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "C"])
def test_coexistence(dcfm, name):
    c = _case(name)
    p = c["P"] * c["g"]
    mask = _mask(name, "random")
    rng = np.random.default_rng(12)
    V, Vp, ynew = rng.standard_normal((p, 3)), rng.standard_normal((p, 2)), rng.standard_normal((p, 2))
    obs = rng.random(p) < 0.6

    def run(plan):
        smp = _open(dcfm, name, mask, burnin=RBURN, mcmc=RN - RBURN, thin=RTHIN, asm_batch=RBATCH, sigma_m2=True,
                    precision_mean=True)
        try:
            smp.set_trace(RN)
            smp.set_probes(V)
            smp.set_precision_probes(Vp)
            smp.set_predict(ynew, obs)
            for first, n in plan:
                smp.run(first, n)
            out = _read(smp)
            out["trace"], out["probes"] = smp.get_trace(), smp.probe_draws()
            out["prec_q"], out["prec_ld"] = smp.precision_draws()
            out["pred"] = smp.predict_raw()
        finally:
            smp.close()
        return out
    one, stepped = run(R_ONE), run(R_STEPPED)
    _assert_same(stepped, one, f"{name} every feature on: stepped vs one call")
    plain = _once(("replay_one", name), lambda: _run_plan(dcfm, name, mask, R_ONE))
    _assert_same(one, plain, f"{name}: the other features moved the imputation")
    assert one["trace"].shape == (RN, 4) and one["probes"].shape == (3, 3, 3) and one["pred"][5] == 3
    for f in ("trace", "probes", "prec_q", "prec_ld"):
        assert np.all(np.isfinite(one[f])) and np.array_equal(stepped[f], one[f]), f
    for a, b in zip(stepped["pred"][:5], one["pred"][:5]):
        assert np.array_equal(a, b)


# ---- 9 ---------------------------------------------------------------------------------------------
def _parity(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return abs(a.mean() - b.mean()) / np.sqrt(a.var(ddof=1) / a.size + b.var(ddof=1) / b.size)


def test_it_imputes(dcfm):
    fx = json.loads((Path(__file__).resolve().parent / "golden" / "missing_chain.json").read_text())
    C = mc.CHAIN
    assert fx["settings"]["nmiss"] == C["nmiss"] and tuple(fx["settings"]["seeds"]) == C["seeds"]
    cc = mc.chain_case()
    assert int(cc["mask"].sum()) == C["nmiss"]
    # the data and the initial state as the driver forms them from the same Y and initial draws (the fixture's
    # differ from them by rounding at most), so that the driver's chain below is the first Sampler chain bit for bit
    Yk, _, _, _, _, keep = dcfm.preprocess_missing(cc["Y"], cc["g"], cc["K"] * cc["g"])
    Yd, mask = dcfm.partition_standardize_missing(Yk, cc["g"], np.asarray(cc["init"].varind))
    assert keep.size == cc["p"] and np.array_equal(mask, cc["mask"]) and np.allclose(Yd, cc["Yd"], rtol=1e-12, atol=1e-12)
    st = dcfm.initial_state(cc["n"], cc["P"], cc["K"], cc["g"], cc["rho"], dcfm.Hyper(), cc["init"])
    init = {f: v for f, v in st.items() if f != "eta"}
    for f, v in init.items():
        assert np.allclose(v, getattr(cc["st"], f).reshape(v.shape), rtol=1e-13), f
    rs, cs, first = [], [], None
    for seed in C["seeds"]:
        smp = dcfm.Sampler(cc["n"], cc["P"], cc["g"], cc["K"], cc["rho"], C["burnin"], C["mcmc"], C["thin"], seed=seed)
        try:
            smp.set_data(Yd)
            smp.set_missing(mask)
            smp.set_state(init)
            smp.run(1, C["burnin"] + C["mcmc"])
            im = smp.imputed()
        finally:
            smp.close()
        assert im["count"] == C["mcmc"] // C["thin"]
        r, c = mc.score(im["mean"], im["sd_total"], cc["truth"], cc["mask"])
        rs.append(r)
        cs.append(c)
        first = im if first is None else first
    print("MISSING_IMPUTES r", [f"{x:.4f}" for x in rs], "c", [f"{x:.4f}" for x in cs],
          "ref r", [f"{x:.4f}" for x in fx["r"]], "ref c", [f"{x:.4f}" for x in fx["c"]])
    assert max(rs) <= 0.80 and min(cs) >= 0.95
    zr, zc = _parity(rs, fx["r"]), _parity(cs, fx["c"])
    print(f"MISSING_IMPUTES parity z: r {zr:.2f}, c {zc:.2f}")
    assert zr < 3.3 and zc < 3.3
    # the driver: the same chain (host initial draws, the first seed), its output in the data's units
    out = dcfm.divideconquer(cc["Y"], cc["g"], cc["K"] * cc["g"], C["burnin"], C["mcmc"], C["thin"], cc["rho"],
                             seed=C["seeds"][0], init_draws=cc["init"], impute=True, return_info=True)
    imp, info = out[1], out[2]
    assert np.array_equal(info["varind"], cc["init"].varind) and imp["count"] == first["count"]
    hole = np.isnan(cc["Y"])
    assert np.array_equal(imp["mean"][~hole], cc["Y"][~hole]) and not np.isnan(imp["mean"]).any()
    assert np.array_equal(imp["sd"] > 0, hole)                              # its NaN positions are the mask
    mean, sd = dcfm.observed_moments(cc["Y"])
    want = dcfm.unstandardize_imputation(first, cc["Y"], mean, sd, info["keep"], info["varind"])
    assert np.allclose(imp["mean"], want["mean"], rtol=1e-12, atol=1e-12)
    assert np.allclose(imp["sd"], want["sd"], rtol=1e-12, atol=1e-12)
