"""The smallest shapes on the device: P < 8 variables per shard and n < 16 rows, down to P = 1 and n = 2
(tests/tiny_shapes.py: the case list and the edges each case reaches; tests/test_tiny_shapes.py measures the
reference at every case on the CPU).  Every bar is one the project already uses; none is new.

  stage-wise parity      every case, default mode: test_gpu_k_paths._check itself (one iteration per call, the
                         oracle restarted from the device's own previous state; X, Z, eta, psi, delta, tau, Plam at
                         1e-10; loading draw backward error <= 1e-13 and the scaled measure against its class bar;
                         ps, omega per row against dc:169 within max(1e-10, residual_rounding_bound);
                         saved_samples() == 2; Sigmaout exactly symmetric and within 1e-12 of the host sum of
                         assemble_sample over the device's own saved states).  At P = 1, K >= 2 the delta / tau
                         comparison is against MATLAB's scalar sum(mat) (quirk Q14, oracle.dc_oracle).
  residual modes         DCFM_FLAG_GUARD_ALL and DCFM_FLAG_EXACT_RESIDUAL at tiny_shapes.MODE_CASES, the same
                         assertions; the guard's fallback agrees with the exact launch within twice the bound.
  unfused                DCFM_FLAG_UNFUSED at tiny_shapes.UNFUSED_CASES (k_prep, k_wpass, k_zdraw, k_colsum, k_delta).
  generated draws        bit for bit the injected chain on the variates at the same counters
                         (tests/test_gpu_generated_draws.py's method; delta_G's shapes contain P).
  two loopback ranks     state and rank 0's Sigmaout bitwise the one-rank run's (tests/test_gpu_loopback.py's pattern).
  ingest and init        set_data_raw and init_state at P g = 3, 4 and 10 columns (four per k_colstats block) and
                         n - 1 = 1, to tests/test_gpu_ingest.py's and tests/test_gpu_init.py's references and bars;
                         yy: sum_i Yd^2 per column at 1e-13, and through the default mode's ps (the SS identity reads
                         yy) against dc:169 in the sweep from the device's own ingest.
  n = 1                  preprocess_device rejects it (dc:57), as the host paths do (tests/test_oracle.py).
  second moment          sigma_m2 at tiny_shapes.M2_CASES with tests/test_gpu_sigma_moments.py's _Ref and _check.
  trace                  at tiny_shapes.TRACE_CASES against tests/test_gpu_trace.py's _oracle_rows.  A sum of logs may
                         sit near zero, so no relative bar on the sum: |got - want| <= 1e-10 sum |summands|, the
                         forward bound of a sum.

The per-feature read-outs (probes, precision, loglik, predict, regression, missing, corr, partial corr, precision
mean, second moment, sigma_apply, sigma_eigs, sigma_solve) at these shapes: tests/test_gpu_tiny_readouts.py
(tests/tiny_readouts.py: their own edges and the cases that reach them).

Measured on the MI355X: DESIGN.md section 2, "Smallest shapes".
"""
import threading

import numpy as np
import pytest

import test_gpu_generated_draws as TG
import test_gpu_init as TI
import test_gpu_k_paths as TK
import test_gpu_sigma_moments as TM
import test_gpu_trace as TT
import tiny_shapes as ts
from helpers import (STATE_CMP, rel_err, residual_rounding_bound, scaled_rel_err, stacked_draws, state_dict)
from oracle import dc_oracle as F

pytestmark = pytest.mark.gpu

TOL = TK.TOL              # 1e-10, the project's stage-wise bar
YD_TOL = 1e-13            # tests/test_gpu_ingest.py
INIT_TOL = TI.TOL         # 1e-14
TRACE_TOL = 1e-10         # tests/test_gpu_trace.py


def _record(record_property, worst):
    for f, e in worst.items():
        record_property(f"worst_{f}", e)


@pytest.mark.parametrize("key", ts.CASES, ids=ts.case_id)
def test_stagewise_parity(dcfm, key, record_property):
    _record(record_property, TK._check(dcfm, key, "default", cases=ts))


@pytest.mark.parametrize("mode", ["guard_all", "exact"])
@pytest.mark.parametrize("key", ts.MODE_CASES, ids=ts.case_id)
def test_stagewise_parity_residual_modes(dcfm, key, mode, record_property):
    _record(record_property, TK._check(dcfm, key, mode, cases=ts))


@pytest.mark.parametrize("key", ts.MODE_CASES, ids=ts.case_id)
def test_guard_fallback_agrees_with_exact(dcfm, key):
    c = ts.case(key)
    guard = TK._run(dcfm, key, "guard_all", False, ts)["states"]
    exact = TK._run(dcfm, key, "exact", False, ts)["states"]
    for it in range(1, ts.N_ITER + 1):
        bound = 2.0 * residual_rounding_bound(exact[it], c["Yd"]).T
        for f in ("ps", "omega"):
            e = scaled_rel_err(guard[it][f], exact[it][f], bound, TOL)
            print(f"TINY_SHAPES_GUARD {ts.case_id(key)} guard_all vs exact iter {it}: {f} {e:.3e} (bound max {bound.max():.3e})")
            assert e < TOL, f"{key} iteration {it}: {f} of the guard's fallback vs the exact launch {e:.3e} (bar {TOL:.0e})"


@pytest.mark.parametrize("key", ts.UNFUSED_CASES, ids=ts.case_id)
def test_stagewise_parity_unfused(dcfm, key, record_property):
    _record(record_property, TK._check(dcfm, key, "unfused", cases=ts))


# ---- generated draws ------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ts.GENERATED_CASES, ids=ts.case_id)
def test_generated_equals_injected_at_the_counters(dcfm, key):
    n, P, g, K = key
    TG._generated_vs_injected(dcfm, n, P * g, g, K, 0)


# ---- two loopback ranks ---------------------------------------------------------------------------------

def _whole_run(dcfm, c, key, nranks):
    """The 3-iteration chain in one run() call on `nranks` loopback ranks: per rank the state, and rank 0's Sigmaout."""
    n, P, g, K = key
    G = g // nranks
    draws = stacked_draws(c["src"], 1, ts.N_ITER)
    smps = [dcfm.Sampler(n, P, g, K, c["rho"], ts.BURNIN, ts.MCMC, ts.THIN, inject_draws=True, nranks=nranks, rank=r,
                         device=0) for r in range(nranks)]
    try:
        if nranks > 1:
            dcfm.Sampler.comm_loopback(smps)
        for r, smp in enumerate(smps):
            smp.set_data(c["Yd"][:, :, r * G:(r + 1) * G])
            st = state_dict(c["st"], r * G, G)
            smp.set_state({f: st[f] for f in st if f != "eta"})
            smp.set_draws(draws, 1, ts.N_ITER)
        out, errs = [None] * nranks, []

        def work(r):
            try:
                smps[r].run(1, ts.N_ITER)
                got = smps[r].get_state()
                got["Sig"] = smps[r].get_sigma()          # collective: rank 0 receives
                out[r] = got
            except Exception as e:                        # noqa: BLE001 - surfaced below
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


@pytest.mark.parametrize("key,per_rank", ts.LOOPBACK_CASES, ids=[ts.case_id(k) for k, _ in ts.LOOPBACK_CASES])
def test_two_loopback_ranks_bitwise(dcfm, key, per_rank):
    n, P, g, K = key
    assert g == 2 * per_rank
    c = ts.case(key)
    one = _whole_run(dcfm, c, key, 1)[0]
    two = _whole_run(dcfm, c, key, 2)
    assert two[1]["Sig"] is None
    assert np.array_equal(two[0]["Sig"], one["Sig"]), "rank 0's Sigmaout is not the one-rank Sigmaout bit for bit"
    for f in STATE_CMP:
        if f in ("X", "delta", "tauh"):                 # replicated
            for r in range(2):
                assert np.array_equal(two[r][f], one[f]), f"{f} of rank {r} differs from the one-rank run"
        else:
            both = np.concatenate([two[r][f] for r in range(2)], axis=-1)
            assert np.array_equal(both, one[f]), f"{f} differs from the one-rank run"
    # and the one-rank run is the oracle's chain
    ref = c["st"].copy()
    S_ref = F.run_chain(c["Yd"], ref, c["rho"], c["hyper"], c["src"].iteration, 1, ts.N_ITER, ts.BURNIN, ts.MCMC, ts.THIN)
    assert rel_err(one["Sig"], S_ref) < TOL
    for f in STATE_CMP:
        assert rel_err(one[f], getattr(ref, f)) < TOL, f


# ---- ingest and init ------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ts.INGEST_CASES, ids=ts.case_id)
def test_set_data_raw_and_the_sweep_from_it(dcfm, key):
    """k_colstats with P g = 3, 4, 10 columns (four per block) and n - 1 = 1; then the default-mode sweep from the
    device's own Yd and yy, whose ps (SS identity: yy_j - 2 lam.C + lam E lam') is held to dc:169."""
    n, P, g, K = key
    c = ts.case(key)
    N = ts.N_ITER
    smp = dcfm.Sampler(n, P, g, K, c["rho"], 0, N, 1, inject_draws=True)
    try:
        cols = dcfm.shard_columns(c["keep"], c["init"].varind, P, 0, g)
        sd, ms = smp.set_data_raw(c["Y"], cols)
        Yd = smp.get_data()
        smp.set_state(state_dict(c["st"]))
        smp.set_draws(stacked_draws(c["src"], 1, N), 1, N)
        smp.run(1, N)
        got = smp.get_state()
        S = smp.get_sigma()
    finally:
        smp.close()
    assert Yd.shape == c["Yd"].shape and rel_err(Yd, c["Yd"]) < YD_TOL
    sd_ref = F.partition(c["Y"][:, c["keep"]], g, c["init"].varind).std(axis=0, ddof=1)      # P x g
    assert rel_err(sd, sd_ref) < YD_TOL and ms > 0.0
    # yy: every standardised column has sum_i Yd_ij^2 = n - 1
    yy, yy_ref = np.sum(Yd * Yd, axis=0), np.sum(c["Yd"] * c["Yd"], axis=0)
    assert np.max(np.abs(yy - yy_ref) / yy_ref) < YD_TOL and np.max(np.abs(yy - (n - 1.0))) < YD_TOL * (n - 1.0)
    ref = c["st"].copy()
    Sref = F.run_chain(c["Yd"], ref, c["rho"], c["hyper"], c["src"].iteration, 1, N, 0, N, 1)
    for f in STATE_CMP:
        e = rel_err(got[f], getattr(ref, f))
        print(f"TINY_SHAPES_INGEST {ts.case_id(key)} {f} {e:.3e}")
        assert e < TOL, f"{f} rel err {e:.3e}"
    assert rel_err(S, Sref) < TOL


@pytest.mark.parametrize("key", ts.INGEST_CASES, ids=ts.case_id)
def test_init_state_matches_host_formula(dcfm, key):
    n, P, g, K = key
    rho, seed = 0.5, 1234
    smp = dcfm.Sampler(n, P, g, K, rho, 0, 2, 1, seed=seed)
    try:
        smp.init_state()
        got = smp.get_state()
    finally:
        smp.close()
    want = TI._host_init(dcfm, n, P, g, K, rho, seed)
    for f in TI.FIELDS:
        if f == "Lambda":
            assert not np.any(got[f])
            continue
        assert rel_err(got[f], want[f]) < INIT_TOL, f


def test_preprocess_device_rejects_one_row(dcfm):
    """dc:57: mean / var of a 1 x P x g array reduce along P; k_colstats would divide by n - 1 = 0."""
    Y = np.arange(1.0, 7.0)[None, :]
    with pytest.raises(ValueError, match="dc:57"):
        dcfm.preprocess_device(Y, 3, 3)
    n, p, P, K, keep = dcfm.preprocess_device(np.vstack([Y, Y + 1.0]), 3, 3)
    assert (n, p, P, K) == (2, 6, 2, 1) and keep.size == 6


# ---- second moment --------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ts.M2_CASES, ids=ts.case_id)
def test_second_moment(dcfm, key):
    n, P, g, K = key
    c = ts.case(key)
    ref = TM._Ref(ts.MCMC / ts.THIN)
    smp = TM._injected(dcfm, c, ts.BURNIN, ts.MCMC, ts.THIN, sigma_m2=True)
    try:
        for it in range(1, ts.N_ITER + 1):
            smp.run(it, 1)
            if TM._saved(it, ts.BURNIN, ts.THIN):
                s = smp.get_state(("Lambda", "omega"))
                ref.add(s["Lambda"], s["omega"], c["rho"])
        assert smp.saved_samples() == len(ref.samples) == 2
        M2, SD, mean = smp.get_sigma_moment("m2"), smp.get_sigma_moment("sd"), smp.get_sigma_moment("mean")
        assert np.array_equal(mean, smp.get_sigma())
    finally:
        smp.close()
    assert rel_err(mean, ref.mean) < TOL
    TM._check(M2, SD, ref, f"TINY_SHAPES_M2 {ts.case_id(key)}")


# ---- trace ----------------------------------------------------------------------------------------------

def _abs_rows(c, N):
    """sum |summand| of each of test_gpu_trace._oracle_rows' four sums, per iteration."""
    ref = c["st"].copy()
    rec = []
    F.run_chain(c["Yd"], ref, c["rho"], c["hyper"], c["src"].iteration, 1, N, 0, N, 1, record=rec)
    return np.array([[np.sum(s.Lambda ** 2), np.sum(np.abs(s.omega)), np.sum(np.abs(np.log(s.ps))),
                      np.sum(np.abs(np.log(s.tauh)))] for s in rec])


@pytest.mark.parametrize("key", ts.TRACE_CASES, ids=ts.case_id)
def test_trace(dcfm, key):
    """Rows (sum Lambda^2, sum omega, sum log ps, sum log tau) against the oracle chain's.  sum log may sit near
    zero (at (2, 1, 3, 1) it has three terms of either sign), so the bar is not relative to the sum but to the
    sum of the summands' magnitudes: |got - want| <= 1e-10 sum |summands|, the forward bound of a sum."""
    n, P, g, K = key
    c = ts.case(key)
    N = ts.N_ITER
    smp = dcfm.Sampler(n, P, g, K, c["rho"], 0, N, 1, inject_draws=True)
    try:
        smp.set_data(c["Yd"])
        smp.set_state(state_dict(c["st"]))
        smp.set_draws(stacked_draws(c["src"], 1, N), 1, N)
        smp.set_trace(N)
        smp.run(1, N)
        tr = smp.get_trace()
    finally:
        smp.close()
    want, mass = TT._oracle_rows(c, N), _abs_rows(c, N)
    assert tr.shape == (N, 4)
    ratio = np.abs(tr - want) / mass
    print(f"TINY_SHAPES_TRACE {ts.case_id(key)} max |got - want| / sum |summands| per column:", ratio.max(axis=0))
    assert np.all(np.abs(tr - want) <= TRACE_TOL * mass), (tr, want, mass)
