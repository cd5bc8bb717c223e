"""CPU tests of the on-device solve's boundary (dcfm_sigma_solve): the binding lists and resolves the
symbol with its ten arguments, a null handle is refused with nothing written, the ABI version and the
kernel-id count stay (the change is additive), Sampler.sigma_solve exists, and permute_vectors is the
inverse of unpermute_vectors on the kept rows -- all without a GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "dcfm.h"


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", HEADER.read_text(), re.M)
    assert m, f"{name} not defined in include/dcfm.h"
    return int(m.group(1), 0)


def test_library_resolves_the_new_symbol(dcfm):
    lib = dcfm.load_library()
    assert "dcfm_sigma_solve" in dcfm.EXPORTS
    assert re.search(r"\bint\s+dcfm_sigma_solve\s*\(", HEADER.read_text()), "not declared in include/dcfm.h"
    fn = lib.dcfm_sigma_solve
    assert fn.restype is C.c_int and len(fn.argtypes) == 10


def test_the_change_is_additive(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    assert _define("DCFM_ABI_VERSION") == 2 == lib.dcfm_abi_version()
    assert _define("DCFM_K_COUNT") == _abi.K_COUNT == 15 == len(_abi.KERNEL_IDS)


def test_null_handle_is_invalid(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    buf, x, rel, quad = ((C.c_double * 4)() for _ in range(4))
    it = (C.c_int32 * 4)()
    ms = C.c_double(0.0)
    rc = lib.dcfm_sigma_solve(None, buf, 1, 1e-8, 10, x, rel, it, quad, C.byref(ms))
    assert rc == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert list(x) == list(rel) == list(quad) == [0.0] * 4 and list(it) == [0] * 4 and ms.value == 0.0


def test_sampler_method_exists(dcfm):
    assert callable(dcfm.Sampler.sigma_solve)
    assert "permute_vectors" in dcfm.__all__
    assert "iters < max_iter" in dcfm.Sampler.sigma_solve.__doc__       # what `converged` means is documented


def test_permute_vectors_by_hand(dcfm):
    """The example of test_unpermute_vectors_by_hand: five input variables, column 2 all zero and dropped,
    keep = [0, 1, 3, 4]; varind = [2, 0, 3, 1] puts the kept columns in the order 3, 0, 4, 1 -- row a of
    the result is row cols[a] of B."""
    keep, varind = np.array([0, 1, 3, 4]), np.array([2, 0, 3, 1])
    B = np.array([[20.0, -2.0], [40.0, -4.0], [7.0, 7.0], [10.0, -1.0], [30.0, -3.0]])     # input order
    got = dcfm.permute_vectors(B, keep, varind)
    assert np.array_equal(got, np.array([[10.0, -1.0], [20.0, -2.0], [30.0, -3.0], [40.0, -4.0]]))
    assert np.array_equal(dcfm.permute_vectors(B[:, 0], keep, varind), got[:, 0])
    # round trips on the kept rows, both ways; the dropped row falls away and comes back as the fill
    back = dcfm.unpermute_vectors(got, keep, varind, 5)
    assert np.array_equal(back[[0, 1, 3, 4]], B[[0, 1, 3, 4]]) and np.array_equal(back[2], [0.0, 0.0])
    V = np.array([[1.0, 5.0], [2.0, 6.0], [3.0, 7.0], [4.0, 8.0]])                          # Sigmaout's order
    assert np.array_equal(dcfm.permute_vectors(dcfm.unpermute_vectors(V, keep, varind, 5), keep, varind), V)
    # sd (of the kept columns, Sigmaout's order) divides, and undoes unpermute_vectors' scaling exactly here
    sd = np.array([2.0, 0.5, 4.0, 1.0])
    assert np.array_equal(dcfm.permute_vectors(B, keep, varind, sd=sd),
                          np.array([[5.0, -0.5], [40.0, -4.0], [7.5, -0.75], [40.0, -4.0]]))
    assert np.array_equal(dcfm.permute_vectors(dcfm.unpermute_vectors(V, keep, varind, 5, sd=sd), keep, varind, sd=sd), V)
    with pytest.raises(ValueError):
        dcfm.permute_vectors(np.zeros((4, 2)), keep, varind)            # a row short of the input's columns
    assert "D^-1 S^-1 D^-1" in dcfm.divideconquer.__doc__               # the unstandardised-precision recipe
