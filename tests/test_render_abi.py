"""CPU checks of the render-mix entry point (csrc/render.hip): the library exports it and it reports argument errors
before anything is launched (there is no device here: a launch would come back as a runtime error, not as -1)."""
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


def test_render_mix_is_exported(lib):
    from diffgfdn_amd import _lib
    assert "gfdn_render_mix" in _lib.SIGNATURES
    assert hasattr(lib, "gfdn_render_mix")
    assert lib.gfdn_abi_version() == 8              # purely additive


def test_render_mix_argument_errors(lib):
    p = 4096                                        # any non-null address: nothing may be read or launched
    R, S, n = 3, 5, 100
    ok = dict(d=p, ld_d=n, rows=None, w=p, c=p, ld_c=n, R=R, S=S, n=n, out=2 * p, ld_out=n)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gfdn_render_mix(a["d"], a["ld_d"], a["rows"], a["w"], a["c"], a["ld_c"], a["R"], a["S"], a["n"],
                                   a["out"], a["ld_out"], None)

    for name in ("d", "w", "c", "out"):             # null pointers
        assert call(**{name: None}) == -1, name
    assert call(S=0) == -1
    assert call(R=0) == -1 and call(n=0) == -1 and call(S=-2) == -1
    assert call(ld_out=n - 1) == -1
    assert call(ld_d=n - 1) == -1 and call(ld_c=n - 1) == -1
    assert call(rows=p, out=p) == -1                # a row index with out = d: not the same rows
    assert call(S=33) == -2                         # more than 32 signals per launch: the caller chunks
