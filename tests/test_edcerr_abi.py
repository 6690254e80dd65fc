"""CPU checks of the EDC-error entry point (csrc/edcerr.hip): the library exports it and it reports argument errors before
anything is launched (there is no device here: a launch would come back as a runtime error, not as -1)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from diffgfdn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "diffgfdn_amd", "csrc"), "-j4"])
    return _lib.load()


def test_edc_err_is_exported(lib):
    from diffgfdn_amd import _lib
    assert "gfdn_edc_err" in _lib.SIGNATURES
    assert hasattr(lib, "gfdn_edc_err")
    assert lib.gfdn_abi_version() == _lib.ABI_VERSION == 8          # purely additive


def _call(lib, ok, **kw):
    a = dict(ok, **kw)
    return lib.gfdn_edc_err(a["dk"], a["ld_d"], a["rows"], a["w"], a["ck"], a["ld_c"], a["tdb"], a["ld_t"], a["R"], a["A"],
                            a["S"], a["L"], a["mode"], a["out"], a["ld_o"], None)


def test_edc_err_argument_errors(lib):
    p = 4096                                        # any non-null address: nothing may be read or launched
    R, A, S, L = 3, 2, 5, 100
    err = dict(dk=p, ld_d=L, rows=None, w=p, ck=p, ld_c=L, tdb=p, ld_t=L, R=R, A=A, S=S, L=L, mode=0, out=2 * p, ld_o=A)
    curve = dict(err, tdb=None, ld_t=0, mode=1, ld_o=L)
    for ok in (err, curve):
        for name in ("dk", "out"):                  # null pointers
            assert _call(lib, ok, **{name: None}) == -1, name
        for name in ("R", "A", "L"):                # non-positive sizes
            assert _call(lib, ok, **{name: 0}) == -1 and _call(lib, ok, **{name: -3}) == -1, name
        assert _call(lib, ok, S=-1) == -1
        assert _call(lib, ok, ld_d=L - 1) == -1 and _call(lib, ok, ld_c=L - 1) == -1      # pitches shorter than L
        assert _call(lib, ok, w=None) == -1 and _call(lib, ok, ck=None) == -1             # W without Ck and the reverse
        assert _call(lib, ok, w=None, ck=None) == -1                                      # S > 0 without either
        assert _call(lib, ok, S=0) == -1                                                  # S = 0 with both
        assert _call(lib, ok, S=33) == -2           # more than 32 group signals per launch: the caller renders them first
        assert _call(lib, ok, mode=2) == -1
    assert _call(lib, err, tdb=None) == -1
    assert _call(lib, err, ld_t=L - 1) == -1
    assert _call(lib, err, ld_o=A - 1) == -1        # err (R, A): rows shorter than A
    assert _call(lib, curve, ld_o=L - 1) == -1      # curve (R, A, L): rows shorter than L
