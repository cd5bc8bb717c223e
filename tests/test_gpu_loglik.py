"""Pointwise log-likelihood draws (dcfm_set_loglik / dcfm_get_loglik) on the GPU: every row's
y_i' Sigma(s)^-1 y_i and every log det against the dense solve and slogdet of the sampler's own state of that
saved iteration within the bounds of loglik_cases.bounds (first order in eps kappa; the tested states have
kappa < 1e3 on the CPU with the oracle's chain), the cross-check with the precision draws of the same rows,
determinism, off means off, capacity and reset, the unfused, exact-residual and generated paths, two loopback
ranks, the argument errors and the driver's `loglik=`."""
import ctypes as C

import numpy as np
import pytest

import loglik_cases as lc
import precision_cases as qc
import probe_cases as pc
from helpers import make_case

pytestmark = pytest.mark.gpu

BASE = (30, 60, 3, 3)
# ((n, p, g, K), rho).  The baseline (n below one 16-row MFMA tile pair: padding rows) at rho = 0.5, 0, 1; one
# shard with one factor; P = 37 (no multiple of the 8-column chunk or of 32); n = 130 (two 128-row blocks, the
# second almost empty); twelve shards (two shard groups); K = 33 (KW = 64, a ragged last tile) and 40; K = 100
# and 128 (KW = 128, the largest LDS footprint)
CASES = [(BASE, 0.5), (BASE, 0.0), (BASE, 1.0), ((30, 21, 1, 1), 0.5), ((30, 74, 2, 5), 0.5), ((130, 74, 2, 5), 0.5),
         ((30, 60, 12, 2), 0.5), ((40, 99, 3, 33), 0.5), ((40, 90, 2, 40), 0.5), ((120, 200, 2, 100), 0.5),
         ((120, 200, 2, 128), 0.5)]
_runs = {}


@pytest.fixture(scope="module")
def drawn(dcfm):
    """(shape, rho) -> the stepwise chain's draws and states, computed once and never modified."""
    def get(shape, rho=0.5):
        if (shape, rho) not in _runs:
            _runs[shape, rho] = lc.run_loglik(dcfm, shape, rho=rho)
        return _runs[shape, rho]
    yield get
    _runs.clear()


def _assert_run(r, shape, what):
    n, p = shape[0], shape[1]
    S = len(pc.SAVED)
    assert r["maha"].shape == (S, n) and r["logdet"].shape == (S,) and r["ll"].shape == (S, n) and len(r["states"]) == S
    assert np.array_equal(r["ll"], -0.5 * (p * np.log(2.0 * np.pi) + r["logdet"][:, None] + r["maha"]))
    for s, st in enumerate(r["states"]):
        lc.assert_draw(r["maha"][s], r["logdet"][s], r["Yd"], st, r["rho"], f"{what} draw {s}")


@pytest.mark.parametrize("shape,rho", CASES)
def test_every_draw_matches_the_dense_reference(drawn, shape, rho):
    _assert_run(drawn(shape, rho), shape, f"{shape} rho={rho}")


def test_agrees_with_the_precision_draws_of_the_same_rows(dcfm, drawn):
    """The first rows of get_data() as precision probes on the same chain: the diagonals of their draws against
    maha within the sum of the two bounds, the log det within its bound; turning loglik on changes no byte of
    the precision draws or of the plain probes."""
    shape = (40, 90, 2, 40)
    nr = 32
    W = pc.probe_block(shape[1], 7, seed=6)
    both = lc.run_loglik(dcfm, shape, precision_rows=nr, probes=W, states=False)
    off = lc.run_loglik(dcfm, shape, precision_rows=nr, probes=W, states=False, on=False)
    assert off["maha"].shape == (0, shape[0]) and both["Q"].shape == (len(pc.SAVED), nr, nr)
    assert both["Q"].tobytes() == off["Q"].tobytes() and both["qlogdet"].tobytes() == off["qlogdet"].tobytes()
    assert both["probe"].tobytes() == off["probe"].tobytes() and both["probe"].shape == (len(pc.SAVED), 7, 7)
    full = drawn(shape)
    assert both["maha"].tobytes() == full["maha"].tobytes() and both["logdet"].tobytes() == full["logdet"].tobytes()
    n, p, g, K = shape
    P = p // g
    for s, st in enumerate(full["states"]):
        qd, _, kappa = lc.dense(full["Yd"], st["Lambda"], st["omega"], full["rho"])
        bl, bld = lc.bounds(qd, kappa, P, K, g)
        bq = 4.0 * (P + K + g + nr) * lc.EPS * kappa * np.abs(qd)       # precision_cases.bounds on the diagonal
        d = np.abs(both["Q"][s].diagonal() - both["maha"][s, :nr])
        print(f"draw {s}: max diff / (sum of the bounds) {np.max(d / (bl[:nr] + bq[:nr])):.4f}")
        assert np.all(d <= bl[:nr] + bq[:nr])
        assert abs(both["qlogdet"][s] - both["logdet"][s]) <= bld


def test_deterministic(dcfm, drawn):
    for shape in (BASE, (40, 90, 2, 40)):
        a = drawn(shape)
        b = lc.run_loglik(dcfm, shape, states=False)         # in one run call: the same chain
        assert a["maha"].tobytes() == b["maha"].tobytes() and a["logdet"].tobytes() == b["logdet"].tobytes()


def test_off_means_off(dcfm):
    n, p, g, K = BASE
    c = make_case(n, p, g, K, seed=21, k0=4)
    sig = []
    for on in (False, True):
        smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], pc.BURNIN, pc.MCMC, pc.THIN, seed=11)
        try:
            smp.set_data(c["Yd"])
            smp.init_state()
            ll, maha, ld = smp.loglik_draws(parts=True)
            assert ll.shape == (0, n) and maha.shape == (0, n) and ld.shape == (0,)
            if on:
                smp.set_loglik()
                assert smp.loglik_draws().shape == (0, n)    # nothing recorded yet
            smp.run(1, pc.N)
            ll, maha, ld = smp.loglik_draws(parts=True)
            S = len(pc.SAVED) if on else 0
            assert ll.shape == (S, n) and maha.shape == (S, n) and ld.shape == (S,)
            assert np.all(np.isfinite(ll)) and np.all(maha > 0)
            sig.append(smp.get_sigma())
        finally:
            smp.close()
    assert np.array_equal(sig[0], sig[1])                    # the same Philox chain, bit for bit


def test_capacity_and_reset(dcfm, drawn):
    full = drawn(BASE)
    r = lc.run_loglik(dcfm, BASE, capacity=2, states=False, keep=True)
    smp = r["smp"]
    try:
        assert r["maha"].shape == (2, BASE[0]) and np.array_equal(r["maha"], full["maha"][:2])
        assert np.array_equal(r["logdet"], full["logdet"][:2])
        smp.set_loglik(4)                                    # again: resets the count
        assert smp.loglik_draws().shape == (0, BASE[0])
        smp.set_loglik(0)                                    # off
        smp.run(2, 1)                                        # a saved iteration with recording off
        assert smp.loglik_draws().shape == (0, BASE[0])
    finally:
        smp.close()


@pytest.mark.parametrize("path", ["unfused", "exact_residual"])
def test_other_launch_paths(dcfm, path):
    from dcfm_amd import _abi
    flags = {"unfused": _abi.DCFM_FLAG_UNFUSED, "exact_residual": _abi.DCFM_FLAG_EXACT_RESIDUAL}[path]
    _assert_run(lc.run_loglik(dcfm, BASE, flags=flags), BASE, path)


def test_generated_draws(dcfm):
    n, p, g, K = BASE
    c = make_case(n, p, g, K, seed=21, k0=4)
    smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], pc.BURNIN, pc.MCMC, pc.THIN, seed=11)
    try:
        smp.set_data(c["Yd"])
        smp.init_state()
        smp.set_loglik()
        sts = []
        for it in range(1, pc.N + 1):
            smp.run(it, 1)
            if it in pc.SAVED:
                sts.append(smp.get_state(("Lambda", "omega")))
        ll, maha, ld = smp.loglik_draws(parts=True)
    finally:
        smp.close()
    _assert_run({"ll": ll, "maha": maha, "logdet": ld, "states": sts, "Yd": c["Yd"], "rho": c["rho"]}, BASE, "generated")


def test_two_loopback_ranks(dcfm):
    shape = (60, 400, 4, 5)
    out, c = lc.loopback_loglik(dcfm, *shape)
    (ll0, q0, l0), (ll1, q1, l1) = out
    assert q0.shape == (len(pc.SAVED), shape[0]) and l0.shape == (len(pc.SAVED),)
    assert q0.tobytes() == q1.tobytes() and l0.tobytes() == l1.tobytes() and ll0.tobytes() == ll1.tobytes()
    one = lc.run_loglik(dcfm, shape, case_seed=23)
    for s, st in enumerate(one["states"]):
        lc.assert_draw(q0[s], l0[s], one["Yd"], st, one["rho"], f"two ranks against the one-rank state, draw {s}")
        lc.assert_draw(one["maha"][s], one["logdet"][s], one["Yd"], st, one["rho"], f"one rank, draw {s}")


def test_argument_errors_leave_the_setting_intact(dcfm, drawn):
    from dcfm_amd import _abi
    full = drawn(BASE)
    n = BASE[0]
    c = make_case(*BASE, seed=21, k0=4)
    smp = pc.start(dcfm, c, BASE[2], BASE[3])
    lib, DP = smp.lib, C.POINTER(C.c_double)
    try:
        smp.set_loglik()
        assert lib.dcfm_set_loglik(smp.h, -1) == _abi.DCFM_ERR_INVALID
        assert lib.dcfm_get_loglik(smp.h, None, None, None) == _abi.DCFM_ERR_INVALID
        assert b"null argument" in lib.dcfm_last_error(smp.h)
        smp.run(1, pc.N)                                     # the setting made before is the one recorded
        _, maha, ld = smp.loglik_draws(parts=True)
        assert np.array_equal(maha, full["maha"]) and np.array_equal(ld, full["logdet"])
        cnt = C.c_int64(-1)
        assert lib.dcfm_get_loglik(smp.h, None, None, C.byref(cnt)) == _abi.DCFM_OK and cnt.value == len(pc.SAVED)
        only = np.zeros(len(pc.SAVED))                       # maha null, logdet alone
        assert lib.dcfm_get_loglik(smp.h, None, only.ctypes.data_as(DP), C.byref(cnt)) == _abi.DCFM_OK
        assert np.array_equal(only, ld)
        qs = np.zeros((len(pc.SAVED), n))                    # logdet null, maha alone
        assert lib.dcfm_get_loglik(smp.h, qs.ctypes.data_as(DP), None, C.byref(cnt)) == _abi.DCFM_OK
        assert np.array_equal(qs, maha)
    finally:
        smp.close()


def test_driver_loglik(dcfm):
    n, p0, g, K = 30, 61, 3, 2
    rng = np.random.default_rng(31)
    Y = rng.standard_normal((n, p0))
    Y[:, 17] = 0.0                                           # dropped: p = 60
    burnin, mcmc, thin = 2, 6, 2
    S, llk, info = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, 0.5, seed=5, loglik=True, return_info=True)
    assert set(llk) == {"ll", "logdet", "waic"} and llk["ll"].shape == (mcmc // thin, n)
    assert llk["logdet"].shape == (mcmc // thin,) and np.all(np.isfinite(llk["ll"]))
    assert np.isfinite(llk["waic"]["waic"]) and np.isfinite(llk["waic"]["se"]) and llk["waic"]["p_waic"] >= 0
    S0, _ = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, 0.5, seed=5, return_info=True)
    assert np.array_equal(S, S0)                             # Sigmaout does not see the recording
    Sr, prc, llk2, _ = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, 0.5, seed=5, precision_probes=Y[0],
                                          loglik=True, return_info=True)
    assert set(prc) == {"draws", "logdet", "mean", "sd"}     # the precision dict, then the loglik dict, then info
    assert np.array_equal(llk2["ll"], llk["ll"]) and np.array_equal(S, Sr)
    # the manual path: the same seed through the Sampler
    keep, varind = info["keep"], info["varind"]
    smp = dcfm.Sampler(n, info["P"], g, info["K"], 0.5, burnin, mcmc, thin, seed=5)
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, varind, info["P"], 0, g))
        smp.init_state()
        smp.set_loglik()
        smp.run(1, burnin + mcmc)
        ll, _, ld = smp.loglik_draws(parts=True)
        assert np.array_equal(ll, llk["ll"]) and np.array_equal(ld, llk["logdet"])
        assert np.array_equal(smp.get_sigma(), S)
    finally:
        smp.close()
