"""The MEX gateway's `sigma_solve` command (matlab/dcfm_mex.c) through the mock MEX runtime
(tests/mexmock).  CPU: malformed calls -- wrong argument counts, a missing or bad handle, a tol or
max_iter that is out of range, fractional or of the wrong class -- are rejected with their error ids
before the library sees a pointer.  GPU: a B of the wrong shape is refused against the handle's own p,
and the command returns what the Python host twin returns, bit for bit (the pointers and sizes go
through unchanged; the int32 steps come back as doubles)."""
import numpy as np
import pytest

from helpers import make_case, stacked_draws, state_dict
from mexmock import driver as mm


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    return mm.Mex(mm.build(tmp_path_factory.mktemp("mexmock_solve")))


def test_malformed_calls_are_rejected(mex):
    B = np.zeros((4, 1))
    for args in ((), (0.0,), (0.0, B, 1e-8, 5.0, 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_solve", *args, nlhs=3)             # h, B and at most tol, max_iter
        assert e.value.id == "dcfm:nargs", args
    for h in (7.0, -1.0, 0.5, 64.0):                           # no such handle
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_solve", h, B)
        assert e.value.id == "dcfm:handle", h
    with pytest.raises(mm.MexError) as e:
        mex.call("sigma_solve", np.zeros(2), B)                # handle not a scalar
    assert e.value.id == "dcfm:arg"
    bad = [(0.0,), (-1e-8,), (np.nan,), (np.inf,), ("tol",), (np.zeros(2),),         # tol
           (1e-8, 0.0), (1e-8, 2.5), (1e-8, -3.0), (1e-8, 2.0 ** 40), (1e-8, "5")]   # max_iter
    for args in bad:
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_solve", 0.0, B, *args, nlhs=3)     # checked before the handle is looked up
        assert e.value.id == "dcfm:arg", args
    assert mex.locks() == 0


@pytest.mark.gpu
def test_command_through_the_gateway_matches_the_host_twin(mex, dcfm):
    n, p, g, K = 40, 48, 4, 5
    burnin, mcmc, thin = 1, 3, 1
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=11)
    P = c["P"]
    st = state_dict(c["st"])
    d = stacked_draws(c["src"], 1, N)
    cfg = dict(n=float(n), P=float(P), g=float(g), K=float(K), rho=c["rho"], burnin=float(burnin),
               mcmc=float(mcmc), thin=float(thin), inject=1.0)
    rng = np.random.default_rng(8)
    B = rng.standard_normal((p, 35))                           # two chunks inside the call
    h = mex.call("create", cfg)
    try:
        mex.call("set_data", h, c["Yd"])
        mex.call("set_state", h, st["Lambda"], st["ps"], st["omega"], st["psi"], st["Plam"], st["X"], st["Z"],
                 st["delta"], st["tauh"])
        mex.call("set_draws", h, d["NZ"], d["NX"], d["NL"], d["Gpsi"], d["Gdelta"], d["Gps"], 1.0, float(N))
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_solve", h, B, nlhs=3)              # no saved sample yet: the library refuses
        assert e.value.id == "dcfm:call" and "saved sample" in e.value.msg
        mex.call("run", h, 1.0, float(N))
        for badB in (np.zeros((p + 1, 2)), np.zeros((p - 1, 1)), np.zeros((p, 0)), B.astype(np.int64), "B"):
            with pytest.raises(mm.MexError) as e:
                mex.call("sigma_solve", h, badB)               # never reaches the library
            assert e.value.id == "dcfm:arg"
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_solve", h, mex.arr(B, cplx=True), raw=(1,))
        assert e.value.id == "dcfm:arg"
        X3, rel3, it3 = mex.call("sigma_solve", h, B, nlhs=3)
        x1 = mex.call("sigma_solve", h, B[:, 3])               # a column vector, one output
        Xc, relc, itc = mex.call("sigma_solve", h, B[:, :5], 1e-6, 4.0, nlhs=3)
    finally:
        mex.call("destroy", h)
    assert mex.locks() == 0

    smp = dcfm.Sampler(n, P, g, K, c["rho"], burnin, mcmc, thin, inject_draws=True)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in st.items() if f != "eta"})
        smp.set_draws(d, 1, N)
        smp.run(1, N)
        refX, ref = smp.sigma_solve(B, return_info=True)
        refc, infoc = smp.sigma_solve(B[:, :5], tol=1e-6, max_iter=4, return_info=True)
    finally:
        smp.close()
    assert X3.shape == (p, 35) and np.array_equal(X3, refX)
    assert rel3.shape == (35, 1) and np.array_equal(rel3[:, 0], ref["relres"])
    assert it3.shape == (35, 1) and np.array_equal(it3[:, 0], ref["iters"])
    assert np.all(ref["relres"] <= 1e-8) and np.all(ref["iters"] > 0)      # a real solve went through
    assert x1.shape == (p, 1) and np.array_equal(x1[:, 0], refX[:, 3])
    assert np.array_equal(Xc, refc) and np.array_equal(relc[:, 0], infoc["relres"])
    assert np.array_equal(itc[:, 0], infoc["iters"]) and np.all(itc <= 4)
