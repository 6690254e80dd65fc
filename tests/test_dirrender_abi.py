"""CPU checks of the directional-render entry point (csrc/dirrender.hip): the library exports it and it reports argument
errors before anything is launched (there is no device here: a launch would come back as a runtime error, not as -1 / -2)."""
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


def test_dir_render_is_exported(lib):
    from diffgfdn_amd import _lib
    assert "gfdn_dir_render" in _lib.SIGNATURES
    assert hasattr(lib, "gfdn_dir_render")
    assert lib.gfdn_abi_version() == 8              # purely additive


def test_dir_render_argument_errors(lib):
    p = 4096                                        # any non-null address: nothing may be read or launched
    ok = dict(w=p, c=2 * p, ld_c=100, a=3 * p, R=3, S=5, Ls=4, J=6, n=100, out=4 * p, ld_out=100)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gfdn_dir_render(a["w"], a["c"], a["ld_c"], a["a"], a["R"], a["S"], a["Ls"], a["J"], a["n"], a["out"],
                                   a["ld_out"], None)

    for name in ("w", "c", "out"):                  # null pointers (a = NULL is the ambisonic mode)
        assert call(**{name: None}) == -1, name
    for name in ("R", "S", "Ls", "n", "J"):         # non-positive sizes; J counts only with a
        assert call(**{name: 0}) == -1 and call(**{name: -2}) == -1, name
    assert call(ld_c=99) == -1 and call(ld_out=99) == -1
    assert call(S=33) == -2 and call(Ls=17) == -2 and call(J=33) == -2
    assert call(a=None, S=33) == -2 and call(a=None, Ls=17) == -2
    assert call(a=None, S=0) == -1 and call(a=None, out=None) == -1
