"""The MEX gateway's `precision_mean` command (matlab/dcfm_mex.c) through the mock MEX runtime
(tests/mexmock).  CPU: malformed calls — missing or bad handle, a column range that is negative, fractional
or of the wrong class — are rejected with their error ids before the library sees a pointer.  GPU: the
command returns what the Python host twin returns, bit for bit, for the whole matrix and for a column
range, refuses a range past p, and without cfg.precision_mean passes the library's refusal on."""
import numpy as np
import pytest

from helpers import make_case, stacked_draws, state_dict
from mexmock import driver as mm


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    return mm.Mex(mm.build(tmp_path_factory.mktemp("mexmock_pm")))


def test_malformed_precision_mean_calls_are_rejected(mex):
    with pytest.raises(mm.MexError) as e:
        mex.call("precision_mean")                             # no handle
    assert e.value.id == "dcfm:nargs"
    with pytest.raises(mm.MexError) as e:
        mex.call("precision_mean", 0.0, 0.0)                   # col0 without ncols
    assert e.value.id == "dcfm:nargs"
    with pytest.raises(mm.MexError) as e:
        mex.call("precision_mean", 0.0, 0.0, 1.0, 2.0)         # one argument too many
    assert e.value.id == "dcfm:nargs"
    for h in (7.0, -1.0, 0.5, 64.0):                           # no such handle
        with pytest.raises(mm.MexError) as e:
            mex.call("precision_mean", h)
        assert e.value.id == "dcfm:handle", h
    with pytest.raises(mm.MexError) as e:
        mex.call("precision_mean", np.zeros(2))                # handle not a scalar
    assert e.value.id == "dcfm:arg"
    for c0, nc in ((-1.0, 4.0), (0.0, -2.0), (0.5, 4.0), (0.0, 1.5), (np.zeros(2), 1.0), ("0", 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("precision_mean", 0.0, c0, nc)            # bad column range
        assert e.value.id == "dcfm:arg", (c0, nc)
    assert mex.locks() == 0


@pytest.mark.gpu
def test_precision_mean_through_the_gateway_matches_the_host_twin(mex, dcfm):
    n, p, g, K = 40, 48, 4, 5
    burnin, mcmc, thin = 1, 3, 1
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=11)
    P = c["P"]
    st = state_dict(c["st"])
    d = stacked_draws(c["src"], 1, N)
    cfg = dict(n=float(n), P=float(P), g=float(g), K=float(K), rho=c["rho"], burnin=float(burnin),
               mcmc=float(mcmc), thin=float(thin), inject=1.0)

    def feed(h):
        mex.call("set_data", h, c["Yd"])
        mex.call("set_state", h, st["Lambda"], st["ps"], st["omega"], st["psi"], st["Plam"], st["X"], st["Z"],
                 st["delta"], st["tauh"])
        mex.call("set_draws", h, d["NZ"], d["NX"], d["NL"], d["Gpsi"], d["Gdelta"], d["Gps"], 1.0, float(N))

    got = {}
    h = mex.call("create", dict(cfg, precision_mean=1.0))
    try:
        feed(h)
        assert not mex.call("precision_mean", h).any()         # no saved sample yet: zeros
        mex.call("run", h, 1.0, float(N))
        got["T"] = mex.call("precision_mean", h)
        got["cols"] = mex.call("precision_mean", h, 5.0, 9.0)
        got["S"] = mex.call("get_sigma", h)
        for c0, nc in ((0.0, float(p + 1)), (float(p), 1.0), (40.0, 9.0)):
            with pytest.raises(mm.MexError) as e:
                mex.call("precision_mean", h, c0, nc)          # past p: never reaches the library
            assert e.value.id == "dcfm:arg"
    finally:
        mex.call("destroy", h)
    h = mex.call("create", cfg)                                # without cfg.precision_mean
    try:
        with pytest.raises(mm.MexError) as e:
            mex.call("precision_mean", h)
        assert e.value.id == "dcfm:call" and "DCFM_FLAG_PRECISION_MEAN" in e.value.msg
    finally:
        mex.call("destroy", h)
    assert mex.locks() == 0

    smp = dcfm.Sampler(n, P, g, K, c["rho"], burnin, mcmc, thin, inject_draws=True, precision_mean=True)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in st.items() if f != "eta"})
        smp.set_draws(d, 1, N)
        smp.run(1, N)
        T, S = smp.get_precision_mean(), smp.get_sigma()
    finally:
        smp.close()
    assert got["T"].shape == (p, p) and np.array_equal(got["T"], T) and np.array_equal(got["S"], S)
    assert np.array_equal(got["cols"], T[:, 5:14])
    assert np.all(T.diagonal() > 0)
