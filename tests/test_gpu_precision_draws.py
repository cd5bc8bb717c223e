"""Per-sample draws of V' Sigma(s)^-1 V and log det Sigma(s) (dcfm_set_precision_probes /
dcfm_get_precision_draws) on the GPU: every draw and every log det against the dense solve and slogdet of
the sampler's own state of that saved iteration within the derived bounds (precision_cases.bounds: first
order in eps kappa; the tested states have kappa < 1e3, verified on the CPU with the oracle's chain, so the
bounds stay below 1e-9 relative), bitwise symmetry, determinism, off means off, capacity and reset,
coexistence with the V' Sigma V probes, two loopback ranks, the argument errors and the driver's
`precision_probes=`."""
import ctypes as C

import numpy as np
import pytest

import precision_cases as qc
import probe_cases as pc
from helpers import make_case

pytestmark = pytest.mark.gpu

BASE = (30, 60, 3, 3)
# ((n, p, g, K), nv, rho).  The baseline at every width (nv = 0: the log det alone; 32: the widest panel);
# one shard of 21 rows with one factor (two uneven slices; no slice is ever empty: a slice holds at least
# 8 rows); P = 37 (four slices, none a multiple of the 4-row MFMA step); twelve shards (two shard groups);
# K = 40 (three tile rows, B_m in 12.5 KiB of LDS); K = 33 (a ragged last tile); K = 100 (78 KiB of LDS, the
# largest footprint short of 128); rho = 0 and rho = 1 (the oracle's chain is finite at rho = 1 here)
CASES = [(BASE, 0, 0.5), (BASE, 1, 0.5), (BASE, 5, 0.5), (BASE, 32, 0.5), ((30, 21, 1, 1), 5, 0.5),
         ((30, 74, 2, 5), 5, 0.5), ((30, 60, 12, 2), 5, 0.5), ((40, 90, 2, 40), 5, 0.5), ((40, 99, 3, 33), 5, 0.5),
         ((120, 200, 2, 100), 5, 0.5), (BASE, 5, 0.0), (BASE, 5, 1.0)]
_runs = {}


@pytest.fixture(scope="module")
def drawn(dcfm):
    """(shape, nv, rho) -> the stepwise chain's draws and states, computed once and never modified."""
    def get(shape, nv, rho=0.5):
        if (shape, nv, rho) not in _runs:
            V = pc.probe_block(shape[1], nv)
            _runs[shape, nv, rho] = (V, qc.run_precision(dcfm, shape, V, rho=rho))
        return _runs[shape, nv, rho]
    yield get
    _runs.clear()


def _assert_draw(Q, ld, V, st, rho, what):
    rq, rl, kappa = qc.ratios(Q, ld, V, st, rho)
    print(f"{what}: kappa {kappa:.3e}, Q max err / bound {rq:.4f}, log det err / bound {rl:.5f}")
    assert np.all(np.isfinite(Q)) and np.isfinite(ld)
    assert kappa <= 1e6, f"{what}: kappa {kappa:.3e}"
    assert rq <= 1.0, f"{what}: Q is {rq:.3f} of its bound"
    assert rl <= 1.0, f"{what}: log det is {rl:.3f} of its bound"


@pytest.mark.parametrize("shape,nv,rho", CASES)
def test_every_draw_matches_the_dense_reference(drawn, shape, nv, rho):
    V, r = drawn(shape, nv, rho)
    S = len(pc.SAVED)
    assert r["Q"].shape == (S, nv, nv) and r["logdet"].shape == (S,) and len(r["states"]) == S
    for s, st in enumerate(r["states"]):
        _assert_draw(r["Q"][s], r["logdet"][s], V, st, rho, f"{shape} nv={nv} rho={rho} draw {s}")
    if nv >= 3:                                              # the all-zero probe: exact zeros
        assert not r["Q"][:, 1, :].any() and not r["Q"][:, :, 1].any()
    assert np.array_equal(r["Q"], np.swapaxes(r["Q"], 1, 2))


def test_logdet_does_not_depend_on_the_probes(drawn):
    """The Gram's K x K corner sees the same operations whatever nv, as long as the slice count (chosen from
    the padded width K + nv) is the same: nv = 0, 1, 5 all pad to 16 here (nv = 32 takes one slice, not two)."""
    ld = [drawn(BASE, nv)[1]["logdet"] for nv in (0, 1, 5)]
    assert all(np.array_equal(ld[0], x) for x in ld[1:])


def test_deterministic(dcfm, drawn):
    for shape, nv in ((BASE, 32), ((40, 90, 2, 40), 5)):
        V, a = drawn(shape, nv)
        b = qc.run_precision(dcfm, shape, V, states=False)   # in one run call: the same chain
        assert a["Q"].tobytes() == b["Q"].tobytes() and a["logdet"].tobytes() == b["logdet"].tobytes()


def test_off_means_off(dcfm):
    n, p, g, K = BASE
    c = make_case(n, p, g, K, seed=21, k0=4)
    sig = []
    for on in (False, True):
        smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], pc.BURNIN, pc.MCMC, pc.THIN, seed=11)
        try:
            smp.set_data(c["Yd"])
            smp.init_state()
            if on:
                smp.set_precision_probes(pc.probe_block(p, 4))
            else:
                Q, ld = smp.precision_draws()
                assert Q.shape == (0, 0, 0) and ld.shape == (0,)
            smp.run(1, pc.N)
            Q, ld = smp.precision_draws()
            assert Q.shape == ((len(pc.SAVED), 4, 4) if on else (0, 0, 0)) and ld.shape == (len(pc.SAVED) if on else 0,)
            sig.append(smp.get_sigma())
        finally:
            smp.close()
    assert np.array_equal(sig[0], sig[1])                    # the same Philox chain, bit for bit


def test_capacity_and_reset(dcfm, drawn):
    shape, nv = BASE, 5
    V, full = drawn(shape, nv)
    r = qc.run_precision(dcfm, shape, V, capacity=2, states=False, keep=True)
    smp = r["smp"]
    try:
        assert r["Q"].shape == (2, nv, nv) and np.array_equal(r["Q"], full["Q"][:2])
        assert np.array_equal(r["logdet"], full["logdet"][:2])
        smp.set_precision_probes(V[:, :2], 4)                # again: replaces V and resets the count
        Q, ld = smp.precision_draws()
        assert Q.shape == (0, 2, 2) and ld.shape == (0,)
        smp.set_precision_probes(None)                       # off
        assert smp.precision_draws()[0].shape[0] == 0
        smp.run(2, 1)                                        # a saved iteration with recording off
        assert smp.precision_draws()[1].shape[0] == 0
    finally:
        smp.close()


def test_coexists_with_the_probes(dcfm, drawn):
    shape, nv = BASE, 5
    V, alone = drawn(shape, nv)
    W = pc.probe_block(shape[1], 7, seed=6)
    both = qc.run_precision(dcfm, shape, V, probes=W, states=False)
    only = pc.run_probed(dcfm, shape, W, states=False)
    assert both["probe"].shape == (len(pc.SAVED), 7, 7) and both["probe"].tobytes() == only["draws"].tobytes()
    assert both["Q"].tobytes() == alone["Q"].tobytes() and both["logdet"].tobytes() == alone["logdet"].tobytes()


def test_two_loopback_ranks(dcfm):
    shape, nv = (60, 400, 4, 5), 7
    V = pc.probe_block(shape[1], nv, seed=9)
    out, c = qc.loopback_precision(dcfm, V, *shape)
    (Q0, l0), (Q1, l1) = out
    assert Q0.shape == (len(pc.SAVED), nv, nv) and l0.shape == (len(pc.SAVED),)
    assert Q0.tobytes() == Q1.tobytes() and l0.tobytes() == l1.tobytes()   # identical bytes on both ranks
    assert np.array_equal(Q0, np.swapaxes(Q0, 1, 2)) and not Q0[:, 1, :].any()
    one = qc.run_precision(dcfm, shape, V, case_seed=23)
    for s, st in enumerate(one["states"]):
        _assert_draw(Q0[s], l0[s], V, st, one["rho"], f"two ranks against the one-rank state, draw {s}")
        _assert_draw(one["Q"][s], one["logdet"][s], V, st, one["rho"], f"one rank, draw {s}")


def test_argument_errors_leave_the_block_intact(dcfm, drawn):
    from dcfm_amd import _abi
    shape, nv = BASE, 5
    V, full = drawn(shape, nv)
    p = shape[1]
    c = make_case(*shape, seed=21, k0=4)
    smp = pc.start(dcfm, c, shape[2], shape[3])
    lib, DP = smp.lib, C.POINTER(C.c_double)
    try:
        smp.set_precision_probes(V)
        Vf = np.asfortranarray(V)
        bad = Vf.copy(order="F")
        bad[p // 2, 3] = np.nan
        wide = np.zeros((p, 33), order="F")
        for args in ((wide.ctypes.data_as(DP), 33, 3), (Vf.ctypes.data_as(DP), -1, 3), (None, nv, 3),
                     (Vf.ctypes.data_as(DP), nv, -1), (bad.ctypes.data_as(DP), nv, 3)):
            assert lib.dcfm_set_precision_probes(smp.h, *args) == _abi.DCFM_ERR_INVALID, args[1:]
        assert lib.dcfm_set_precision_probes(smp.h, None, nv, 3) == _abi.DCFM_ERR_INVALID
        assert b"null argument" in lib.dcfm_last_error(smp.h)
        cnt = C.c_int64(-1)
        assert lib.dcfm_get_precision_draws(smp.h, None, None, None) == _abi.DCFM_ERR_INVALID
        smp.run(1, pc.N)                                     # the block set before is the one recorded
        Q, ld = smp.precision_draws()
        assert np.array_equal(Q, full["Q"]) and np.array_equal(ld, full["logdet"])
        assert lib.dcfm_get_precision_draws(smp.h, None, None, C.byref(cnt)) == _abi.DCFM_OK and cnt.value == len(pc.SAVED)
        only = np.zeros(len(pc.SAVED))                       # Q null, logdet alone
        assert lib.dcfm_get_precision_draws(smp.h, None, only.ctypes.data_as(DP), C.byref(cnt)) == _abi.DCFM_OK
        assert np.array_equal(only, ld)
    finally:
        smp.close()


def test_driver_precision_probes(dcfm):
    n, p0, g, K = 30, 61, 3, 2
    rng = np.random.default_rng(31)
    Y = rng.standard_normal((n, p0))
    Y[:, 17] = 0.0                                           # dropped: p = 60
    V = rng.standard_normal((p0, 4))
    burnin, mcmc, thin = 2, 6, 2
    S, prc, info = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, 0.5, seed=5, precision_probes=V,
                                      return_info=True)
    assert set(prc) == {"draws", "logdet", "mean", "sd"} and prc["draws"].shape == (mcmc // thin, 4, 4)
    assert prc["logdet"].shape == (mcmc // thin,)
    Sr, prb, prc2, _ = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, 0.5, seed=5, probes=V[:, 0],
                                          precision_probes=V[:, 0], return_info=True)
    assert set(prb) == {"draws", "mean", "sd"}               # the probes dict, then the precision dict, then info
    assert np.array_equal(prc2["logdet"], prc["logdet"]) and np.array_equal(S, Sr)
    assert np.array_equal(prc["mean"], prc["draws"].mean(axis=0)) and np.array_equal(prc["sd"], prc["draws"].std(axis=0))
    hd = dcfm.heldout_log_density(prc["draws"], prc["logdet"], info["p"])
    assert hd["per_sample"].shape == (mcmc // thin, 4) and np.all(np.isfinite(hd["lppd"]))
    # the manual path: the same seed through the Sampler
    keep, varind = info["keep"], info["varind"]
    Vp = dcfm.permute_vectors(V, keep, varind)
    smp = dcfm.Sampler(n, info["P"], g, info["K"], 0.5, burnin, mcmc, thin, seed=5)
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, varind, info["P"], 0, g))
        smp.init_state()
        smp.set_precision_probes(Vp)
        smp.run(1, burnin + mcmc)
        Q, ld = smp.precision_draws()
        assert np.array_equal(Q, prc["draws"]) and np.array_equal(ld, prc["logdet"])
        assert np.array_equal(smp.get_sigma(), S)
    finally:
        smp.close()
