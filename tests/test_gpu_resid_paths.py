"""Every path of the residual-precision update (dc:168-171, csrc/resid.h) against dc:169 as written, at
shapes small enough to run in a second: the default SS identity, its guard's fallbacks (resid_rows8
inside k_lambda for K <= 32; k_resid_flagged for K > 32) and the exact-residual launches (k_resid64,
k_resid<64>, k_resid<128>) all end in the same ps / omega formula and, but for the identity, the
same residual arithmetic.  Injected draws, 2 iterations: the first forms the loading systems from the
caller's Plam, the second from psi o tau.

Shapes (n, P, g, K), each chosen for a place these kernels can go wrong:
  (37, 19, 3,  7)  narrow, k_lambda<8>; P no multiple of 8 (a partial last wave: lanes without a row,
                   lanes without a residual column); n far below NP, so the mask of padding rows is live
  (37, 45, 2, 30)  narrow, k_lambda<30>; PP = 64, so k_resid64's second column pair is part padding
  (40, 45, 3, 40)  wide, KW = 64; two 32-row tiles, the second partial
  (40, 33, 2, 70)  wide, KW = 128, five 16-column blocks of the loading system
Modes: default; DCFM_FLAG_EXACT_RESIDUAL; DCFM_FLAG_GUARD_ALL (the guard rejects every row); for the narrow
shapes the last two also through the side-stream layout (DCFM_FLAG_UNFUSED: the k_draws variates).

After each iteration, no row excluded:
  * ps and omega per row, unscaled relative, <= 1e-10 (the project's bar) against oracle.dc_oracle.update_ps
    applied to the GPU's own eta and Lambda (helpers.ps_direct_err);
  * the guard's fallback and the exact launch agree per row within twice helpers.residual_rounding_bound
    at that state (two correct evaluations of dc:169 in different summation orders; the docstring there
    derives the factor), measured with helpers.scaled_rel_err.
The reference needs no GPU: test_reference_in_range checks on the CPU that it stays finite and positive."""
import functools

import numpy as np
import pytest

from helpers import make_case, ps_direct_err, residual_rounding_bound, scaled_rel_err, stacked_draws, state_dict
from oracle import dc_oracle as F

TOL = 1e-10
N_ITER = 2
SHAPES = [(37, 19, 3, 7), (37, 45, 2, 30), (40, 45, 3, 40), (40, 33, 2, 70)]
UNFUSED, EXACT, GUARD_ALL = 0x2, 0x10, 0x40     # include/dcfm.h
MODES = {"default": 0, "exact": EXACT, "guard_all": GUARD_ALL,
         "unfused_exact": UNFUSED | EXACT, "unfused_guard_all": UNFUSED | GUARD_ALL}


def _modes(shape):
    return [m for m in MODES if shape[3] <= 32 or not m.startswith("unfused")]


def _id(shape):
    return "n%d_P%d_g%d_K%d" % shape


@functools.lru_cache(maxsize=None)
def _case(shape):
    n, P, g, K = shape
    c = make_case(n, P * g, g, K, seed=5)
    assert (c["n"], c["P"]) == (n, P), "preprocessing dropped a column"
    return c


@functools.lru_cache(maxsize=None)
def _gpu_states(shape, mode):
    """The state after each of the N_ITER iterations of `mode` (computed once, shared, read only)."""
    import __graft_entry__ as ge
    dcfm = ge.load_package()
    n, P, g, K = shape
    c = _case(shape)
    smp = dcfm.Sampler(n, P, g, K, c["rho"], N_ITER, 1, 1, inject_draws=True, flags=MODES[mode])
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in state_dict(c["st"]).items() if f != "eta"})
        smp.set_draws(stacked_draws(c["src"], 1, N_ITER), 1, N_ITER)
        out = []
        for it in range(1, N_ITER + 1):
            smp.run(it, 1)
            out.append(smp.get_state())
        return out
    finally:
        smp.close()


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_reference_in_range(shape):
    c = _case(shape)
    ref = c["st"].copy()
    for it in range(1, N_ITER + 1):
        F.gibbs_iteration(ref, c["Yd"], c["rho"], c["hyper"], c["src"].iteration(it))
        for f in ("ps", "omega"):
            v = getattr(ref, f)
            assert np.all(np.isfinite(v)) and np.all(v > 0.0), f"{shape} iter {it}: reference {f} out of range"


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", [(s, m) for s in SHAPES for m in _modes(s)],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else v)
def test_ps_omega_against_residual(shape, mode):
    c = _case(shape)
    for it, got in enumerate(_gpu_states(shape, mode), start=1):
        e = ps_direct_err(got, c["st"], c["Yd"], c["hyper"], c["src"].iteration(it))
        print(f"{_id(shape)} {mode} iter {it}: ps / omega vs dc:169 residual, per row {e:.3e}")
        assert e < TOL, f"{shape} {mode} iter {it}: ps / omega vs dc:169 residual, per row {e:.3e} (bar {TOL:.0e})"


@pytest.mark.gpu
@pytest.mark.parametrize("shape,pre", [(s, p) for s in SHAPES for p in ("", "unfused_") if s[3] <= 32 or not p],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else (v or "fused_"))
def test_guard_fallback_agrees_with_exact(shape, pre):
    c = _case(shape)
    guard, exact = _gpu_states(shape, pre + "guard_all"), _gpu_states(shape, pre + "exact")
    for it in range(1, N_ITER + 1):
        bound = 2.0 * residual_rounding_bound(exact[it - 1], c["Yd"]).T       # P x g, the ps / omega layout
        for f in ("ps", "omega"):
            e = scaled_rel_err(guard[it - 1][f], exact[it - 1][f], bound, TOL)
            print(f"{_id(shape)} {pre}guard_all vs exact iter {it}: {f} {e:.3e} (bound max {bound.max():.3e})")
            assert e < TOL, f"{shape} iter {it}: {f} of the guard's fallback vs the exact launch {e:.3e} (bar {TOL:.0e})"
