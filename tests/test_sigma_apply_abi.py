"""CPU tests of the Sigmaout-operator boundary (dcfm_sigma_apply, dcfm_sigma_eigs): the binding lists
and resolves both symbols, a null handle is refused, the ABI version and the kernel-id count stay
(the change is additive), and unpermute_vectors puts rows back in the input's order -- all without
a GPU."""
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


def test_library_resolves_the_new_symbols(dcfm):
    lib = dcfm.load_library()
    text = HEADER.read_text()
    for name in ("dcfm_sigma_apply", "dcfm_sigma_eigs"):
        assert name in dcfm.EXPORTS
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"{name} not declared in include/dcfm.h"
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes
    assert len(lib.dcfm_sigma_apply.argtypes) == 5 and len(lib.dcfm_sigma_eigs.argtypes) == 9


def test_the_change_is_additive(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    assert _define("DCFM_ABI_VERSION") == 2 == lib.dcfm_abi_version()
    assert _define("DCFM_K_COUNT") == _abi.K_COUNT == 15 == len(_abi.KERNEL_IDS)


def test_null_handle_is_invalid(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    buf = (C.c_double * 4)()
    n = C.c_int32(0)
    assert lib.dcfm_sigma_apply(None, buf, 1, buf, None) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert lib.dcfm_sigma_eigs(None, 1, 1e-8, 4, 1, buf, buf, buf, C.byref(n)) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert n.value == 0 and list(buf) == [0.0] * 4                      # nothing written


def test_unpermute_vectors_by_hand(dcfm):
    """Five input variables, column 2 all zero and dropped: keep = [0, 1, 3, 4]; varind = [2, 0, 3, 1]
    puts the kept columns in the order 3, 0, 4, 1 -- row a of V belongs to input variable cols[a]."""
    keep, varind = np.array([0, 1, 3, 4]), np.array([2, 0, 3, 1])
    assert list(dcfm.output_columns(keep, varind)) == [3, 0, 4, 1]
    V = np.array([[10.0, -1.0], [20.0, -2.0], [30.0, -3.0], [40.0, -4.0]])
    got = dcfm.unpermute_vectors(V, keep, varind, 5)
    assert np.array_equal(got, np.array([[20.0, -2.0], [40.0, -4.0], [0.0, 0.0], [10.0, -1.0], [30.0, -3.0]]))
    nan = dcfm.unpermute_vectors(V[:, 0], keep, varind, 5, fill=np.nan)
    assert nan.shape == (5,) and np.isnan(nan[2]) and list(nan[[0, 1, 3, 4]]) == [20.0, 40.0, 10.0, 30.0]
    sd = np.array([2.0, 0.5, 3.0, 1.0])                                 # of the kept columns, Sigmaout's order
    scaled = dcfm.unpermute_vectors(V, keep, varind, 5, sd=sd)
    assert np.array_equal(scaled, np.array([[10.0, -1.0], [40.0, -4.0], [0.0, 0.0], [20.0, -2.0], [90.0, -9.0]]))
    # the row analogue of unpermute_sigma: (S V) unpermuted = unpermute(S) unpermute(V), exactly here
    S = np.array([[4.0, 1.0, 0.0, 2.0], [1.0, 3.0, 1.0, 0.0], [0.0, 1.0, 2.0, 1.0], [2.0, 0.0, 1.0, 5.0]])
    lhs = dcfm.unpermute_vectors(S @ V, keep, varind, 5)
    assert np.array_equal(lhs, dcfm.unpermute_sigma(S, keep, varind, 5) @ got)
    with pytest.raises(ValueError):
        dcfm.unpermute_vectors(np.zeros((5, 2)), keep, varind, 5)
    assert "no longer orthonormal" in dcfm.unpermute_vectors.__doc__


def test_sampler_methods_exist(dcfm):
    assert callable(dcfm.Sampler.sigma_apply) and callable(dcfm.Sampler.sigma_eigs)
    assert "unpermute_vectors" in dcfm.__all__
