"""The MEX gateway's `set_precision_probes` and `precision_draws` commands (matlab/dcfm_mex.c) through the
mock MEX runtime (tests/mexmock).  CPU: malformed calls -- wrong argument counts, a missing or bad handle,
a capacity that is negative, fractional or of the wrong class -- are rejected with their error ids before
the library sees a pointer.  GPU: a V of the wrong shape is refused against the handle's own p, a p x 0
block records the log det alone, and `precision_draws` returns what the Python host twin returns,
transposed into MATLAB's order, bit for bit."""
import numpy as np
import pytest

from helpers import make_case, stacked_draws, state_dict
from mexmock import driver as mm


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    return mm.Mex(mm.build(tmp_path_factory.mktemp("mexmock_precision")))


def test_malformed_calls_are_rejected(mex):
    V = np.zeros((4, 2))
    for args in ((), (0.0,), (0.0, V, 2.0, 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("set_precision_probes", *args)            # h, V and at most capacity
        assert e.value.id == "dcfm:nargs", args
    for args in ((), (0.0, 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("precision_draws", *args)                 # takes exactly h
        assert e.value.id == "dcfm:nargs", args
    for h in (7.0, -1.0, 0.5, 64.0):                           # no such handle
        with pytest.raises(mm.MexError) as e:
            mex.call("set_precision_probes", h, V)
        assert e.value.id == "dcfm:handle", h
        with pytest.raises(mm.MexError) as e:
            mex.call("precision_draws", h)
        assert e.value.id == "dcfm:handle", h
    with pytest.raises(mm.MexError) as e:
        mex.call("precision_draws", np.zeros(2))               # handle not a scalar
    assert e.value.id == "dcfm:arg"
    for cap in (-1.0, 2.5, np.nan, "3", np.zeros(2)):
        with pytest.raises(mm.MexError) as e:
            mex.call("set_precision_probes", 0.0, V, cap)      # checked before the handle is looked up
        assert e.value.id == "dcfm:arg", cap
    assert mex.locks() == 0


@pytest.mark.gpu
def test_commands_through_the_gateway_match_the_host_twin(mex, dcfm):
    n, p, g, K = 40, 48, 4, 5
    burnin, mcmc, thin = 1, 4, 2
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=11)
    P = c["P"]
    st = state_dict(c["st"])
    d = stacked_draws(c["src"], 1, N)
    cfg = dict(n=float(n), P=float(P), g=float(g), K=float(K), rho=c["rho"], burnin=float(burnin),
               mcmc=float(mcmc), thin=float(thin), inject=1.0)
    V = np.random.default_rng(8).standard_normal((p, 6))
    h = mex.call("create", cfg)
    try:
        mex.call("set_data", h, c["Yd"])
        mex.call("set_state", h, st["Lambda"], st["ps"], st["omega"], st["psi"], st["Plam"], st["X"], st["Z"],
                 st["delta"], st["tauh"])
        mex.call("set_draws", h, d["NZ"], d["NX"], d["NL"], d["Gpsi"], d["Gdelta"], d["Gps"], 1.0, float(N))
        Q, ld = mex.call("precision_draws", h, nlhs=2)         # nothing set
        assert Q.shape == (0, 0, 0) and ld.size == 0
        for badV in (np.zeros((p + 1, 2)), np.zeros((p - 1, 1)), np.zeros((p, 33)), V.astype(np.int64), "V"):
            with pytest.raises(mm.MexError) as e:
                mex.call("set_precision_probes", h, badV)      # never reaches the library
            assert e.value.id == "dcfm:arg"
        with pytest.raises(mm.MexError) as e:
            mex.call("set_precision_probes", h, mex.arr(V, cplx=True), raw=(1,))
        assert e.value.id == "dcfm:arg"
        Vn = V.copy()
        Vn[5, 1] = np.inf
        with pytest.raises(mm.MexError) as e:
            mex.call("set_precision_probes", h, Vn)            # the library refuses a non-finite entry
        assert e.value.id == "dcfm:call" and "finite" in e.value.msg
        mex.call("set_precision_probes", h, V)                 # default capacity mcmc / thin
        mex.call("run", h, 1.0, float(N))
        Q, ld = mex.call("precision_draws", h, nlhs=2)
        assert mex.call("precision_draws", h).shape == Q.shape  # one output: Q
        mex.call("set_precision_probes", h, np.zeros((p, 0)), 1.0)   # the log det alone, capacity 1: the count resets
        assert mex.call("precision_draws", h).shape == (0, 0, 0)
        mex.call("run", h, 2.0, 1.0)                           # one more saved iteration
        Q0, ld0 = mex.call("precision_draws", h, nlhs=2)
        assert Q0.shape == (0, 0, 1) and ld0.size == 1 and np.isfinite(ld0).all()
        mex.call("set_precision_probes", h, V, 0.0)            # off
        assert mex.call("precision_draws", h).shape == (0, 0, 0)
    finally:
        mex.call("destroy", h)
    assert mex.locks() == 0

    smp = dcfm.Sampler(n, P, g, K, c["rho"], burnin, mcmc, thin, inject_draws=True)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in st.items() if f != "eta"})
        smp.set_draws(d, 1, N)
        smp.set_precision_probes(V)
        smp.run(1, N)
        ref, rld = smp.precision_draws()
    finally:
        smp.close()
    assert ref.shape == (mcmc // thin, 6, 6) and np.all(np.isfinite(ref)) and np.all(ref.diagonal(axis1=1, axis2=2) > 0)
    assert Q.shape == (6, 6, mcmc // thin) and np.array_equal(Q, np.transpose(ref, (2, 1, 0)))
    assert np.array_equal(np.asarray(ld).reshape(-1), rld)
