"""Per-sample draws of V' Sigma(s) V (dcfm_set_probes / dcfm_get_probe_draws) on the GPU: every draw
against the sampler's own state of that saved iteration within the dot-product rounding bound, the
draws' mean against the Sigmaout operator, their spread against the on-device second moment, off means
off, capacity and reset, determinism and bitwise symmetry, two loopback ranks, the argument errors and
the driver's `probes=`."""
import ctypes as C

import numpy as np
import pytest

import probe_cases as pc
from helpers import make_case

pytestmark = pytest.mark.gpu

# (n, p, g, K): three shards; one shard of 21 rows with one factor (32 slices: uneven and empty row
# ranges); P = 37; K > 32 (the kp = 64 layout); twelve shards (fewer than 32 slices per shard)
SHAPES = [((30, 60, 3, 3), 1), ((30, 60, 3, 3), 5), ((30, 60, 3, 3), 32), ((30, 21, 1, 1), 5),
          ((30, 74, 2, 5), 5), ((40, 90, 2, 40), 5), ((30, 60, 12, 2), 5)]
_runs = {}


@pytest.fixture(scope="module")
def probed(dcfm):
    """(shape, nv) -> the stepwise chain's draws and states, computed once and never modified."""
    def get(shape, nv):
        if (shape, nv) not in _runs:
            V = pc.probe_block(shape[1], nv)
            _runs[shape, nv] = (V, pc.run_probed(dcfm, shape, V))
        return _runs[shape, nv]
    yield get
    _runs.clear()


def _assert_within(got, want, bound, what):
    err = np.abs(got - want)
    print(f"{what}: max err {err.max():.3e}, max err / bound {np.max(err / np.where(bound > 0, bound, 1.0)):.3f}")
    assert np.all(err <= bound), f"{what}: {err.max():.3e} against {bound.max():.3e}"


@pytest.mark.parametrize("shape,nv", SHAPES)
def test_every_draw_matches_the_samplers_own_state(probed, shape, nv):
    V, r = probed(shape, nv)
    assert r["draws"].shape == (len(pc.SAVED), nv, nv) and len(r["states"]) == len(pc.SAVED)
    for s, st in enumerate(r["states"]):
        Q, bound = pc.host_draw(V, st["Lambda"], st["omega"], r["rho"])
        assert np.all(np.isfinite(r["draws"][s]))
        _assert_within(r["draws"][s], Q, bound, f"{shape} nv={nv} draw {s}")
    if nv >= 3:                                              # the all-zero probe: exact zeros
        assert not r["draws"][:, 1, :].any() and not r["draws"][:, :, 1].any()


def test_mean_agrees_with_sigma_apply(dcfm):
    shape, nv = (30, 74, 2, 5), 5
    V = pc.probe_block(shape[1], nv)
    r = pc.run_probed(dcfm, shape, V, keep=True)
    try:
        SV = r["smp"].sigma_apply(V)
    finally:
        r["smp"].close()
    bound = sum(pc.host_draw(V, st["Lambda"], st["omega"], r["rho"])[1] for st in r["states"]) / pc.EFFSAMP
    _assert_within(r["draws"].sum(axis=0) / pc.EFFSAMP, V.T @ SV, bound, "mean of the draws")


def test_spread_agrees_with_the_second_moment(dcfm):
    shape = (30, 60, 3, 3)                                   # P = 20: rows 3 and 17 in shard 0, 45 in shard 2
    idx = [3, 17, 45]
    V = np.zeros((shape[1], 3))
    V[idx, range(3)] = 1.0
    r = pc.run_probed(dcfm, shape, V, states=False, keep=True, sigma_m2=True)
    try:
        sd = r["smp"].get_sigma_moment("sd")
        m2 = r["smp"].get_sigma_moment("m2")
        saved = r["smp"].saved_samples()
    finally:
        r["smp"].close()
    assert saved == len(pc.SAVED) == r["draws"].shape[0]
    M2 = m2[np.ix_(idx, idx)] * (pc.EFFSAMP / saved)
    var = r["draws"].var(axis=0)                             # population form, as DCFM_SIGMA_SD
    # M2 - mean^2 cancels: the read-out's stated accuracy is absolute in M2, on the variance
    _assert_within(sd[np.ix_(idx, idx)] ** 2, var, 64.0 * pc.EPS * M2, "variance of the unit-probe draws")
    assert np.all(var.diagonal() > 0)


def test_off_means_off(dcfm):
    n, p, g, K = 30, 60, 3, 3
    c = make_case(n, p, g, K, seed=21, k0=4)
    sig = []
    for probes in (False, True):
        smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], pc.BURNIN, pc.MCMC, pc.THIN, seed=11)
        try:
            smp.set_data(c["Yd"])
            smp.init_state()
            if probes:
                smp.set_probes(pc.probe_block(p, 4))
            else:
                assert smp.probe_draws().shape[0] == 0
            smp.run(1, pc.N)
            q = smp.probe_draws()
            assert q.shape == ((len(pc.SAVED), 4, 4) if probes else (0, 0, 0))
            sig.append(smp.get_sigma())
        finally:
            smp.close()
    assert np.array_equal(sig[0], sig[1])                    # the same Philox chain, bit for bit


def test_capacity_and_reset(dcfm, probed):
    shape, nv = (30, 60, 3, 3), 5
    V, full = probed(shape, nv)
    r = pc.run_probed(dcfm, shape, V, capacity=2, states=False, keep=True)
    smp = r["smp"]
    try:
        assert r["draws"].shape == (2, nv, nv) and np.array_equal(r["draws"], full["draws"][:2])
        smp.set_probes(V[:, :2], 4)                          # again: replaces V and resets the count
        assert smp.probe_draws().shape == (0, 2, 2)
        smp.set_probes(None)                                 # off
        assert smp.probe_draws().shape[0] == 0
        smp.run(2, 1)                                        # a saved iteration with recording off
        assert smp.probe_draws().shape[0] == 0
    finally:
        smp.close()


def test_deterministic_and_symmetric(dcfm, probed):
    shape, nv = (30, 60, 3, 3), 32
    V, a = probed(shape, nv)
    b = pc.run_probed(dcfm, shape, V, states=False)          # in one run call: the same chain
    assert np.array_equal(a["draws"], b["draws"])
    for (sh, w), (_, r) in list(_runs.items()):
        assert np.array_equal(r["draws"], np.swapaxes(r["draws"], 1, 2)), (sh, w)


def test_two_loopback_ranks(dcfm):
    shape, nv = (60, 400, 4, 5), 7
    V = pc.probe_block(shape[1], nv, seed=9)
    out, c = pc.loopback_probed(dcfm, V, *shape)
    assert out[0].shape == (len(pc.SAVED), nv, nv)
    assert out[0].tobytes() == out[1].tobytes()              # identical bytes on both ranks
    assert np.array_equal(out[0], np.swapaxes(out[0], 1, 2))
    one = pc.run_probed(dcfm, shape, V, case_seed=23)
    for s, st in enumerate(one["states"]):
        Q, bound = pc.host_draw(V, st["Lambda"], st["omega"], one["rho"])
        _assert_within(out[0][s], one["draws"][s], bound, f"two ranks against one, draw {s}")
        _assert_within(out[0][s], Q, bound, f"two ranks against the state, draw {s}")


def test_argument_errors_leave_the_block_intact(dcfm, probed):
    from dcfm_amd import _abi
    shape, nv = (30, 60, 3, 3), 5
    V, full = probed(shape, nv)
    p = shape[1]
    c = make_case(*shape, seed=21, k0=4)
    smp = pc.start(dcfm, c, shape[2], shape[3])
    lib, DP = smp.lib, C.POINTER(C.c_double)
    try:
        smp.set_probes(V)
        Vf = np.asfortranarray(V)
        bad = Vf.copy(order="F")
        bad[p // 2, 3] = np.nan
        wide = np.zeros((p, 33), order="F")
        for args in ((Vf.ctypes.data_as(DP), 0, 3), (wide.ctypes.data_as(DP), 33, 3), (None, nv, 3),
                     (Vf.ctypes.data_as(DP), nv, -1), (bad.ctypes.data_as(DP), nv, 3)):
            assert lib.dcfm_set_probes(smp.h, *args) == _abi.DCFM_ERR_INVALID, args[1:]
        assert lib.dcfm_set_probes(smp.h, None, nv, 3) == _abi.DCFM_ERR_INVALID
        assert b"null argument" in lib.dcfm_last_error(smp.h)
        cnt = C.c_int64(-1)
        assert lib.dcfm_get_probe_draws(smp.h, None, None) == _abi.DCFM_ERR_INVALID
        smp.run(1, pc.N)                                     # the block set before is the one recorded
        assert np.array_equal(smp.probe_draws(), full["draws"])
        assert lib.dcfm_get_probe_draws(smp.h, None, C.byref(cnt)) == _abi.DCFM_OK and cnt.value == len(pc.SAVED)
    finally:
        smp.close()


def test_driver_probes(dcfm):
    n, p0, g, K = 30, 61, 3, 2
    rng = np.random.default_rng(31)
    Y = rng.standard_normal((n, p0))
    Y[:, 17] = 0.0                                           # dropped: p = 60
    V = rng.standard_normal((p0, 4))
    burnin, mcmc, thin = 2, 6, 2
    S, prb, info = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, 0.5, seed=5, probes=V, return_info=True)
    assert set(prb) == {"draws", "mean", "sd"} and prb["draws"].shape == (mcmc // thin, 4, 4)
    Sr, sol, prb2, _ = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, 0.5, seed=5, rhs=V[:, 0], probes=V[:, 0],
                                          return_info=True)
    assert set(sol) == {"x", "relres", "iters", "quad"}      # the rhs dict, then the probes dict, then info
    assert np.array_equal(prb2["draws"][:, 0, 0], prb["draws"][:, 0, 0]) and np.array_equal(S, Sr)
    assert np.array_equal(prb["mean"], prb["draws"].mean(axis=0)) and np.array_equal(prb["sd"], prb["draws"].std(axis=0))
    # the manual path: the same seed through the Sampler
    keep, varind = info["keep"], info["varind"]
    Vp = dcfm.permute_vectors(V, keep, varind)
    assert Vp.shape == (60, 4)
    smp = dcfm.Sampler(n, info["P"], g, info["K"], 0.5, burnin, mcmc, thin, seed=5)
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, varind, info["P"], 0, g))
        smp.init_state()
        smp.set_probes(Vp)
        smp.run(1, burnin + mcmc)
        assert np.array_equal(smp.probe_draws(), prb["draws"])
        assert np.array_equal(smp.get_sigma(), S)
    finally:
        smp.close()
