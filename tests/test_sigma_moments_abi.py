"""CPU tests of the posterior-moment read-out's boundary (DCFM_FLAG_SIGMA_M2,
dcfm_get_sigma_moment[_cols]): the header and the ctypes binding agree on the new constants,
the library exports the two entry points, a null handle is refused, and dcfm_create validates
a configuration with the flag exactly as without it — all without a GPU."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "dcfm.h"


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", HEADER.read_text(), re.M)
    assert m, f"{name} not defined in include/dcfm.h"
    return int(m.group(1), 0)


def test_header_and_binding_agree_on_the_constants(dcfm):
    from dcfm_amd import _abi
    assert _define("DCFM_FLAG_SIGMA_M2") == _abi.DCFM_FLAG_SIGMA_M2 == 0x80
    assert _define("DCFM_SIGMA_MEAN") == _abi.DCFM_SIGMA_MEAN == 0
    assert _define("DCFM_SIGMA_M2") == _abi.DCFM_SIGMA_M2 == 1
    assert _define("DCFM_SIGMA_SD") == _abi.DCFM_SIGMA_SD == 2
    assert _abi.SIGMA_MOMENTS == {"mean": 0, "m2": 1, "sd": 2}
    # the flag is a bit of its own
    others = [v for k, v in vars(_abi).items() if k.startswith("DCFM_FLAG_") and k != "DCFM_FLAG_SIGMA_M2"]
    assert all(v & _abi.DCFM_FLAG_SIGMA_M2 == 0 for v in others)
    # additive: the version and the kernel-id count stay (arrays are sized by the count)
    assert _define("DCFM_ABI_VERSION") == 2 and _define("DCFM_K_COUNT") == _abi.K_COUNT == 15


def test_library_resolves_the_new_symbols(dcfm):
    lib = dcfm.load_library()
    for name in ("dcfm_get_sigma_moment_cols", "dcfm_get_sigma_moment"):
        assert name in dcfm.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
    assert lib.dcfm_abi_version() == 2


def test_null_handle_is_invalid(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    out = (C.c_double * 4)()
    for which in (_abi.DCFM_SIGMA_MEAN, _abi.DCFM_SIGMA_M2, _abi.DCFM_SIGMA_SD, 7):
        assert lib.dcfm_get_sigma_moment_cols(None, which, 0, 1, out) == _abi.DCFM_ERR_INVALID
        assert lib.dcfm_get_sigma_moment(None, which, out) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)


def _create(dcfm, **kw):
    """tests/test_abi.py's _create, restated."""
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    cfg = _abi.DcfmConfig()
    base = dict(n=10, P=4, g=2, K=2, rho=0.5, burnin=0, mcmc=2, thin=1, nranks=1, rank=0, device=0,
                as_=1.0, bs=0.3, df=3.0, ad1=2.0, bd1=1.0, ad2=2.0, bd2=1.0)
    base.update(kw)
    for k, v in base.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    rc = lib.dcfm_create(C.byref(cfg), C.byref(h))
    msg = lib.dcfm_last_error(None).decode()
    if rc == 0:
        lib.dcfm_destroy(h)
    return rc, msg


def test_create_with_the_flag_validates_as_without(dcfm):
    from dcfm_amd import _abi
    M2 = _abi.DCFM_FLAG_SIGMA_M2
    cases = [dict(K=129), dict(g=3, nranks=2), dict(rho=1.5), dict(thin=0), dict(n=0), dict(bs=0.0),
             dict(as_=0.0), dict(ad2=-1.0), dict(g=1024, P=2), dict(), dict(df=1.5), dict(asm_batch=3),
             dict(g=1024, P=2, flags=_abi.DCFM_FLAG_UNFUSED), dict(ad1=0.5, flags=_abi.DCFM_FLAG_INJECT_DRAWS)]
    for kw in cases:
        off = _create(dcfm, **kw)
        on = _create(dcfm, **dict(kw, flags=kw.get("flags", 0) | M2))
        assert on == off, (kw, on, off)
    assert _create(dcfm, rho=1.5, flags=M2)[0] == _abi.DCFM_ERR_INVALID
    assert _create(dcfm, K=129, flags=M2)[0] == _abi.DCFM_ERR_UNSUPPORTED


def test_sampler_rejects_an_unknown_moment_name(dcfm):
    import pytest
    with pytest.raises(ValueError):
        dcfm.Sampler._moment("variance")
    assert [dcfm.Sampler._moment(w) for w in ("mean", "m2", "sd", 1)] == [0, 1, 2, 1]
