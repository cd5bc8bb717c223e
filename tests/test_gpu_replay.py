"""Exact replay of dcfm_run's two schedules (FusedSchedule, SideSchedule; csrc/dcfm.hip) across call,
stream and batch seams.  A generated-draw chain is a function of its seed alone (replay_cases.py), so:

  (a) the chain stepped one iteration per call on ONE stream is the reference's chain at every iteration:
      stage-wise against the CPU oracle restarted from the device's own state, fed the host restatement of
      the Philox variates (oracle.philox_ref.PhiloxSource, not dcfm_rng_fill) -- the trusted chain;
  (b) one multi-stream run, and the same run cut at batch-aligned and at ragged seams (a one-iteration and
      an empty call among them), ends in that chain's state bit for bit; Sigmaout is bitwise where the
      flush grouping is the same and within 1e-12 where the summation order differs;
  (c) the draw-slot cache (gen_first / gen_n, kept across calls) serves hits, short hits and misses;
  (d) two loopback ranks replay the same way, and rank 0's Sigmaout is the one-rank one;
  (e) trace, probes, precision probes, log-likelihood, second moment and precision mean, all on at once,
      give the same per-sample outputs under every plan and do not move the chain;
  (f) profiling changes nothing, and the launch counts are what the schedule code implies.

A missing or misplaced wait in the host code does not fault: it gives a slightly different, still
plausible chain that no tolerance test against the oracle flags.  A passing bitwise comparison shows that
no race showed itself in this run, not that none exists.
"""
import numpy as np
import pytest

import replay_cases as rc
from helpers import (SBW_COND_WELL, SBW_TOL_WELL, STATE_CMP, as_oracle_state as _as_oracle, residual_rounding_bound, scaled_rel_err,
                     stagewise_errors)

pytestmark = pytest.mark.gpu

TOL = 1e-10           # the project's stage-wise bar (tests/test_gpu_excursion.py)
BW_TOL = 1e-13        # loading backward error
SIGMA_ORDER = 1e-12   # Sigmaout under another summation order (test_c3_batch_size_invariance)
# the second moment and the precision mean under another flush grouping: the normwise bar of their own
# test_batched_flush_in_one_run (tests/test_gpu_sigma_moments.py, tests/test_gpu_precision_mean.py)
MOMENT_ORDER = 1e-10
FOUR = ["wide64", "wide128", "unfused", "fused"]

_cache = {}


def _once(key, fn):
    """Reference runs are made once and shared (their arrays read-only)."""
    if key not in _cache:
        r = fn()
        for v in _arrays(r):
            v.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def _arrays(r):
    if isinstance(r, np.ndarray):
        yield r
    elif isinstance(r, dict):
        for v in r.values():
            yield from _arrays(v)
    elif isinstance(r, (list, tuple)):
        for v in r:
            yield from _arrays(v)


def _stepped(dcfm, layout, asm_batch=rc.ASM_BATCH):
    """The trusted chain: 27 calls of one iteration on one stream, synchronised and read after each."""
    return _once(("stepped", layout, asm_batch),
                 lambda: rc.run_plan(dcfm, layout, rc.STEPPED, flags=rc.ONE_STREAM, asm_batch=asm_batch, sync=True,
                                     states=True))


def _one(dcfm, layout):
    return _once(("one", layout), lambda: rc.run_plan(dcfm, layout, rc.ONE))


def _norm_rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _assert_state_equal(got, want, what):
    assert set(got) == set(want) == set(STATE_CMP)              # every STATE_FIELDS member
    for f in want:
        assert np.array_equal(got[f], want[f]), f"{what}: {f} not bitwise equal"


# ---- (a) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", FOUR)
def test_stepped_chain_is_the_references(dcfm, layout, record_property):
    """Measured on the MI355X (worst over the 27 iterations; X, Z, eta, psi, delta, tauh, Plam normwise, ps /
    omega per row against max(1e-10, the residual's rounding bound), loading rows by backward error): see
    DESIGN.md section 2, "Replay invariants".  Every row of these layouts has cond(D Q_j D) <= 1e3 in every
    iteration (tests/test_loading_measure.py: <= 9.6 on the reference's chain), so the diagonally scaled
    backward error is held to SBW_TOL_WELL and the class itself is asserted."""
    from oracle import philox_ref as R
    c = rc.case(layout)
    states = _stepped(dcfm, layout)["states"]
    assert len(states) == rc.N + 1
    src = R.PhiloxSource(rc.CHAIN_SEED, c["n"], c["p"], c["g"], c["K"], c["hyper"])
    worst = {}
    for it in range(1, rc.N + 1):
        got = states[it]
        xmax = float(np.abs(got["X"]).max())
        assert xmax < 10.0, f"iteration {it}: max|X| {xmax:.3g}: the chain left the stationary range"
        errs, bw, ref, (sbw, cond) = stagewise_errors(_as_oracle(states[it - 1]), got, c["Yd"], c["rho"], c["hyper"],
                                                      src.iteration(it), scaled=True)
        bound = residual_rounding_bound(got, c["Yd"]).T
        for f in ("ps", "omega"):
            worst[f + "_raw"] = max(worst.get(f + "_raw", 0.0), errs[f])
            errs[f] = scaled_rel_err(got[f], getattr(ref, f), bound, TOL)
        worst["xmax"] = max(worst.get("xmax", 0.0), xmax)
        worst["lambda_bw"] = max(worst.get("lambda_bw", 0.0), bw)
        worst["lambda_sbw"] = max(worst.get("lambda_sbw", 0.0), float(sbw.max()))
        worst["cond_dqd"] = max(worst.get("cond_dqd", 0.0), float(cond.max()))
        for f, e in errs.items():
            worst[f] = max(worst.get(f, 0.0), e)
        for f, e in errs.items():
            assert e < TOL, f"iteration {it}: stage {f} rel err {e:.3e} (bar {TOL:.0e})"
        assert bw <= BW_TOL, f"iteration {it}: loading backward error {bw:.3e} (bar {BW_TOL:.0e})"
        assert cond.max() <= SBW_COND_WELL, f"iteration {it}: cond(DQD) {cond.max():.3e}: a row left the well class"
        assert sbw.max() <= SBW_TOL_WELL, (f"iteration {it}: scaled loading backward error {sbw.max():.3e} at "
                                           f"{np.unravel_index(np.argmax(sbw), sbw.shape)} (bar {SBW_TOL_WELL:.0e})")
    for f, e in worst.items():
        record_property(f"worst_{f}", e)
    print("REPLAY_STAGEWISE", layout, {k: f"{v:.2e}" for k, v in sorted(worst.items())})


# ---- (b) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", FOUR)
def test_one_run_and_split_runs_are_the_stepped_chain(dcfm, layout):
    stepped = _stepped(dcfm, layout)
    assert stepped["saved"] == 12
    runs = {"ONE": _one(dcfm, layout)}
    for name in ("ALIGNED", "RAGGED"):
        runs[name] = rc.run_plan(dcfm, layout, rc.PLANS[name])
    for name, r in runs.items():
        _assert_state_equal(r["state"], stepped["state"], f"{layout} {name} vs the stepped one-stream chain")
        assert r["saved"] == 12, name
    S = runs["ONE"]["sigma"]
    assert np.all(np.isfinite(S)) and np.array_equal(S, S.T)
    assert np.array_equal(runs["ALIGNED"]["sigma"], S), "ALIGNED flushes as ONE does: Sigmaout must be bitwise"
    for name, r in (("RAGGED", runs["RAGGED"]), ("STEPPED", stepped)):
        e = _norm_rel(r["sigma"], S)
        print(f"REPLAY_SIGMA {layout} {name} vs ONE: {e:.3e}")
        assert e < SIGMA_ORDER, f"{name} vs ONE: Sigmaout rel {e:.3e}"


@pytest.mark.parametrize("layout", FOUR)
def test_single_sample_flushes_are_bitwise(dcfm, layout):
    """asm_batch = 1: every sample is flushed alone, in one run as in the stepped chain, so Sigmaout has
    one summation order; the 12 flushes of the one run ping-pong Lb[0] / Lb[1] through e_free."""
    assert rc.flush_points(rc.ONE, asm_batch=1) == rc.flush_points(rc.STEPPED, asm_batch=1)
    stepped = _stepped(dcfm, layout, asm_batch=1)
    one = rc.run_plan(dcfm, layout, rc.ONE, asm_batch=1)
    assert one["saved"] == stepped["saved"] == 12
    _assert_state_equal(one["state"], stepped["state"], f"{layout} ONE vs STEPPED, asm_batch 1")
    _assert_state_equal(stepped["state"], _stepped(dcfm, layout)["state"], f"{layout} asm_batch 1 vs 2")
    assert np.array_equal(one["sigma"], stepped["sigma"]), "Sigmaout not bitwise equal at asm_batch 1"


# ---- (c) -------------------------------------------------------------------------------------------
def _cache_sequence(dcfm, layout, count_draws):
    """The four steps on one handle; the state after each, and k_draws launches per step with count_draws."""
    c = rc.case(layout)
    init = rc.init_state(c)
    smp = rc._sampler(dcfm, layout, c, flags=0, asm_batch=rc.ASM_BATCH, burnin=100, features=False)
    out, launches = [], []
    try:
        smp.set_data(c["Yd"])
        if count_draws:
            smp.set_profiling_kernels(["k_draws"])
        for calls in ([(1, 12)],                       # 1: fills slot 0 with [1-8], slot 1 with [9-12]
                      [(1, 12)],                       # 2: both slots hit
                      [(1, 5), (6, 7)],                # 3: a hit shorter than the cached batch, then a miss
                      [(1, 3), None, (1, 12)]):        # 4: the cached batch is too short: regenerated
            smp.set_state(init)
            for call in calls:
                if call is None:
                    smp.set_state(init)
                else:
                    smp.run(*call)
            out.append(smp.get_state())
            if count_draws:
                launches.append(smp.kernel_stats()["k_draws"][1])
        assert smp.saved_samples() == 0
    finally:
        smp.close()
    return out, launches


@pytest.mark.parametrize("layout", ["wide64", "unfused"])
def test_draw_slot_cache(dcfm, layout):
    fresh = rc.run_plan(dcfm, layout, [(1, 12)], burnin=100)
    assert fresh["saved"] == 0
    states, _ = _cache_sequence(dcfm, layout, False)
    for i, st in enumerate(states):
        _assert_state_equal(st, fresh["state"], f"{layout} cache step {i + 1} vs a fresh handle")
    # the same with the k_draws launches counted: the steps take the paths they are named for
    states, launches = _cache_sequence(dcfm, layout, True)
    for i, st in enumerate(states):
        _assert_state_equal(st, fresh["state"], f"{layout} cache step {i + 1} (counted) vs a fresh handle")
    assert launches == [12, 12, 12 + 7, 12 + 7 + 3 + 8], launches


# ---- (d) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["wide64", "fused", "unfused30"])
def test_two_ranks_replay(dcfm, layout):
    one = rc.run_plan_ranks(dcfm, layout, rc.ONE, 2)
    ragged = rc.run_plan_ranks(dcfm, layout, rc.RAGGED, 2)
    for r in range(2):
        _assert_state_equal(ragged[r]["state"], one[r]["state"], f"{layout} rank {r}: RAGGED vs ONE")
        assert one[r]["saved"] == ragged[r]["saved"] == 12
    for out, name in ((one, "ONE"), (ragged, "RAGGED")):
        for f in ("X", "delta", "tauh"):
            assert np.array_equal(out[0]["state"][f], out[1]["state"][f]), f"{name}: {f} differs between the ranks"
        assert out[1]["sigma"] is None
    assert np.array_equal(one[0]["sigma"], _one(dcfm, layout)["sigma"]), "rank 0's Sigmaout vs the one-rank run"
    e = _norm_rel(ragged[0]["sigma"], one[0]["sigma"])
    assert e < SIGMA_ORDER, f"two ranks, RAGGED vs ONE: Sigmaout rel {e:.3e}"


# ---- (e) -------------------------------------------------------------------------------------------
PER_SAMPLE = ("trace", "probes", "prec_q", "prec_logdet", "ll_maha", "ll_logdet")


@pytest.mark.parametrize("layout", ["wide64", "fused"])
def test_everything_switched_on(dcfm, layout):
    runs = {name: rc.run_plan(dcfm, layout, plan, features=True,
                              **(dict(flags=rc.ONE_STREAM, sync=True) if name == "STEPPED" else {}))
            for name, plan in rc.PLANS.items()}
    one = runs["ONE"]
    assert one["trace"].shape == (rc.N, 4) and one["probes"].shape == (12, 3, 3)
    assert one["prec_q"].shape == (12, 2, 2) and one["prec_logdet"].shape == (12,)
    assert one["ll_maha"].shape == (12, rc.case(layout)["n"]) and one["ll_logdet"].shape == (12,)
    for f in PER_SAMPLE + ("m2", "prec_mean"):
        assert np.all(np.isfinite(one[f])), f
    chain = _stepped(dcfm, layout)["state"]
    for name, r in runs.items():
        assert r["saved"] == 12
        _assert_state_equal(r["state"], chain, f"{layout} {name} with every feature on vs the plain chain")
        for f in PER_SAMPLE:
            assert np.array_equal(r[f], one[f]), f"{name} vs ONE: per-sample output {f} not bitwise equal"
    for f in ("sigma", "m2", "prec_mean"):
        assert np.array_equal(runs["ALIGNED"][f], one[f]), f"ALIGNED vs ONE: accumulator {f} not bitwise equal"
    assert np.array_equal(one["sigma"], _one(dcfm, layout)["sigma"]), "the features moved Sigmaout"
    for name in ("RAGGED", "STEPPED"):
        for f, bar in (("sigma", SIGMA_ORDER), ("m2", MOMENT_ORDER), ("prec_mean", MOMENT_ORDER)):
            e = _norm_rel(runs[name][f], one[f])
            print(f"REPLAY_FEATURES {layout} {name} vs ONE: {f} {e:.3e}")
            assert e < bar, f"{name} vs ONE: {f} rel {e:.3e} (bar {bar:.0e})"


# ---- (f) -------------------------------------------------------------------------------------------
def _expected_launches(dcfm, layout, plan):
    """KTimer scopes of dcfm_run on one rank (no collectives), from the schedule code in csrc/dcfm.hip."""
    c = rc.case(layout)
    n_saved = len(rc.saved_iterations(plan))
    n_flush = len(rc.flush_points(plan))
    calls = sum(1 for _, n in plan if n > 0)
    want = dict.fromkeys(dcfm._abi.KERNEL_IDS, 0)
    want["k_assemble"] = n_flush                       # flush_batch: one scope per flush
    if c["K"] <= 32 and not (rc.layout_flags(layout) & rc.UNFUSED):
        # FusedSchedule::step: k_wcol, k_xdraw, k_cpass, then loading_rows' k_lambda, which also saves;
        # tail(): one k_delta scope per call that ran an iteration
        for k in ("k_wpass", "k_xdraw", "k_cpass", "k_lambda"):
            want[k] = rc.N
        want["k_delta"] = calls
        return want
    # SideSchedule::step: prep, asum and xchol (both under k_xchol) on the side stream; wpass, zdraw, xred,
    # xdraw, cpass, k_lambda, colsum, delta on the main stream; one k_draws launch per generated iteration
    for k in ("k_prep", "k_wpass", "k_zdraw", "k_xred", "k_xdraw", "k_cpass", "k_lambda", "k_colsum", "k_delta",
              "k_draws"):
        want[k] = rc.N
    want["k_xchol"] = 2 * rc.N
    if c["K"] > 32:
        want["k_resid"] = rc.N                         # loading_rows: k_resid_flagged behind every k_lambda_w
        want["k_save"] = n_saved                       # save_sample: k_save copies Lambda and omega
    return want


@pytest.mark.parametrize("layout", ["wide64", "fused"])
def test_profiling_changes_nothing(dcfm, layout):
    plain = _one(dcfm, layout)
    prof = rc.run_plan(dcfm, layout, rc.ONE, profiling=True)
    _assert_state_equal(prof["state"], plain["state"], f"{layout}: profiled vs unprofiled")
    assert np.array_equal(prof["sigma"], plain["sigma"]), "profiling moved Sigmaout"
    assert len(rc.flush_points(rc.ONE)) == 6 and len(rc.saved_iterations(rc.ONE)) == 12
    want = _expected_launches(dcfm, layout, rc.ONE)
    if layout == "wide64":
        assert all(want[k] == rc.N for k in ("k_lambda", "k_wpass", "k_cpass", "k_draws", "k_resid"))
        assert want["k_save"] == 12 and want["k_assemble"] == 6
    else:
        assert all(want[k] == rc.N for k in ("k_lambda", "k_wpass", "k_cpass")) and want["k_save"] == 0
    assert prof["stats"] == want
