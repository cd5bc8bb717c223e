"""The MEX gateway's `set_regression` and `regression` commands (matlab/dcfm_mex.c) through the mock MEX runtime
(tests/mexmock).  CPU: malformed calls -- missing or bad handle, a response list of the wrong class, too long,
fractional or below 1 -- are rejected with their error ids before the library sees a pointer.  GPU: the seven
outputs are what the Python host twin returns, bit for bit, with 1-based responses; a response past p never
reaches the library, and without cfg.regression the library's refusal is passed on."""
import numpy as np
import pytest

from helpers import make_case, stacked_draws, state_dict
from mexmock import driver as mm


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    return mm.Mex(mm.build(tmp_path_factory.mktemp("mexmock_regression")))


def test_malformed_regression_calls_are_rejected(mex):
    for args in ((), (0.0,), (0.0, np.array([1.0]), 2.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("set_regression", *args)                  # no handle / no list / one too many
        assert e.value.id == "dcfm:nargs", args
    for args in ((), (0.0, 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("regression", *args)                      # the handle, nothing else
        assert e.value.id == "dcfm:nargs", args
    for resp in ("1", np.arange(1.0, 34.0), np.array([0.0]), np.array([1.5]), np.array([2.0, -3.0]),
                 np.array([np.nan]), np.array([1e12])):
        with pytest.raises(mm.MexError) as e:
            mex.call("set_regression", 0.0, resp)              # rejected before the handle is looked up
        assert e.value.id == "dcfm:arg", resp
    for cmd, rest in (("set_regression", (np.array([1.0]),)), ("regression", ())):
        for h in (7.0, -1.0, 0.5, 64.0):                       # no such handle
            with pytest.raises(mm.MexError) as e:
                mex.call(cmd, h, *rest)
            assert e.value.id == "dcfm:handle", (cmd, h)
        with pytest.raises(mm.MexError) as e:
            mex.call(cmd, np.zeros(2), *rest)                  # handle not a scalar
        assert e.value.id == "dcfm:arg", cmd
    assert mex.locks() == 0


@pytest.mark.gpu
def test_regression_through_the_gateway_matches_the_host_twin(mex, dcfm):
    n, p, g, K = 40, 48, 4, 5
    burnin, mcmc, thin = 1, 3, 1
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=11)
    P = c["P"]
    st = state_dict(c["st"])
    d = stacked_draws(c["src"], 1, N)
    R = np.array([30, 2, 47, 13])                              # 0-based
    cfg = dict(n=float(n), P=float(P), g=float(g), K=float(K), rho=c["rho"], burnin=float(burnin),
               mcmc=float(mcmc), thin=float(thin), inject=1.0)

    def feed(h):
        mex.call("set_data", h, c["Yd"])
        mex.call("set_state", h, st["Lambda"], st["ps"], st["omega"], st["psi"], st["Plam"], st["X"], st["Z"],
                 st["delta"], st["tauh"])
        mex.call("set_draws", h, d["NZ"], d["NX"], d["NL"], d["Gpsi"], d["Gdelta"], d["Gps"], 1.0, float(N))

    h = mex.call("create", dict(cfg, regression=1.0))
    try:
        feed(h)
        out = mex.call("regression", h, nlhs=7)                # nothing set: empty arrays, count 0
        assert all(o.size == 0 for o in out[:6]) and float(np.ravel(out[6])[0]) == 0.0
        for bad in (np.array([float(p + 1)]), np.array([1.0, float(p + 3)])):
            with pytest.raises(mm.MexError) as e:
                mex.call("set_regression", h, bad)             # past p: never reaches the library
            assert e.value.id == "dcfm:arg"
        with pytest.raises(mm.MexError) as e:
            mex.call("set_regression", h, np.array([3.0, 9.0, 3.0]))   # a duplicate: the library's refusal
        assert e.value.id == "dcfm:call" and "twice" in e.value.msg
        mex.call("set_regression", h, (R + 1).astype(np.float64))
        out = mex.call("regression", h, nlhs=7)                # no saved sample yet
        assert all(o.size == 0 for o in out[:6]) and float(np.ravel(out[6])[0]) == 0.0
        mex.call("run", h, 1.0, float(N))
        got = mex.call("regression", h, nlhs=7)
        first = mex.call("regression", h)                      # one output: coef alone
        S = mex.call("get_sigma", h)
        mex.call("set_regression", h, np.zeros((0, 0)))        # []: off
        off = mex.call("regression", h, nlhs=7)
        assert off[0].size == 0 and float(np.ravel(off[6])[0]) == 0.0
    finally:
        mex.call("destroy", h)
    h = mex.call("create", cfg)                                # without cfg.regression
    try:
        with pytest.raises(mm.MexError) as e:
            mex.call("set_regression", h, np.array([1.0]))
        assert e.value.id == "dcfm:call" and "DCFM_FLAG_REGRESSION" in e.value.msg
        assert float(np.ravel(mex.call("regression", h, nlhs=7)[6])[0]) == 0.0
    finally:
        mex.call("destroy", h)
    assert mex.locks() == 0

    smp = dcfm.Sampler(n, P, g, K, c["rho"], burnin, mcmc, thin, inject_draws=True, regression=True)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in st.items() if f != "eta"})
        smp.set_draws(d, 1, N)
        smp.set_regression(R)
        smp.run(1, N)
        ref = smp.regression_raw()
        Sref = smp.get_sigma()
    finally:
        smp.close()
    assert np.array_equal(S, Sref) and ref[6] == mcmc == float(np.ravel(got[6])[0])
    for a, b, shape in zip(got[:6], ref[:6], ((p, 4), (p, 4), (4, 4), (4, 4), (4,), (4,))):
        assert np.array_equal(np.reshape(a, shape, order="F"), b)
    assert np.array_equal(np.reshape(first, (p, 4), order="F"), ref[0])
    assert np.any(ref[0] != 0) and not ref[0][R].any()
