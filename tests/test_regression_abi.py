"""CPU tests of the regression read-out's boundary (dcfm_set_regression / dcfm_get_regression): the header and the
ctypes binding agree on the flag and the two calls, and a null handle is refused before any device is touched."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "dcfm.h"


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", HEADER.read_text(), re.M)
    assert m, f"{name} not defined in include/dcfm.h"
    return int(m.group(1), 0)


def test_header_and_binding_agree(dcfm):
    from dcfm_amd import _abi
    assert _define("DCFM_FLAG_REGRESSION") == _abi.DCFM_FLAG_REGRESSION == 0x800
    others = [v for k, v in vars(_abi).items() if k.startswith("DCFM_FLAG_") and k != "DCFM_FLAG_REGRESSION"]
    assert len(others) >= 11 and all(v & _abi.DCFM_FLAG_REGRESSION == 0 for v in others)
    assert _define("DCFM_ABI_VERSION") == 2
    lib = dcfm.load_library()
    vp, DP, IP = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert "dcfm_set_regression" in dcfm.EXPORTS and "dcfm_get_regression" in dcfm.EXPORTS
    assert lib.dcfm_set_regression.restype is C.c_int and lib.dcfm_get_regression.restype is C.c_int
    assert list(lib.dcfm_set_regression.argtypes) == [vp, IP, C.c_int32]
    assert list(lib.dcfm_get_regression.argtypes) == [vp, DP, DP, DP, DP, DP, DP, IP]
    hdr = HEADER.read_text()
    for name in ("dcfm_set_regression", "dcfm_get_regression"):
        assert re.search(rf"^int\s+{name}\(", hdr, re.M), name
    assert lib.dcfm_abi_version() == 2


def test_null_handle_is_invalid(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    resp = (C.c_int64 * 2)(0, 1)
    assert lib.dcfm_set_regression(None, resp, 2) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert lib.dcfm_set_regression(None, None, 0) == _abi.DCFM_ERR_INVALID
    cnt = C.c_int64(-7)
    out = (C.c_double * 4)()
    assert lib.dcfm_get_regression(None, out, None, None, None, None, None, C.byref(cnt)) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert cnt.value == -7 and not any(out)
