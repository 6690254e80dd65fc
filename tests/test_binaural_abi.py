"""CPU checks of the binaural entry points (csrc/binaural.hip): the header declares them, the built library exports them with
the argument counts of the declarations, and they report argument errors before anything is launched (there is no device
here: a launch would come back as a runtime error, not as -1 or -2)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gfdn_binaural_compose", "gfdn_binaural_ola")


@pytest.fixture(scope="module")
def lib():
    from diffgfdn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "diffgfdn_amd", "csrc"), "-j4"])
    return _lib.load()


def test_binaural_entry_points_are_declared_and_exported(lib):
    from diffgfdn_amd import _lib
    header = open(os.path.join(ROOT, "include", "diffgfdn_hip.h")).read()
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is declared in the header"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, f"{name}: the ctypes signature has the header's argument count"
    assert lib.gfdn_abi_version() == _lib.ABI_VERSION == 8          # purely additive


def _compose(lib, ok, **kw):
    a = dict(ok, **kw)
    return lib.gfdn_binaural_compose(a["w"], a["ch"], a["ld_c"], a["S"], a["ah"], a["ld_a"], a["path"], a["row_off"],
                                     a["nrows"], a["rot"], a["hh"], a["ld_h"], a["P"], a["k0"], a["nseg"], a["Kb"], a["Ls"],
                                     a["alpha"], a["b"], a["ld_b"], None)


def test_binaural_compose_argument_errors(lib):
    p = 4096                                        # any non-null address: nothing may be read or launched
    Kb = 257
    bank = dict(w=p, ch=2 * p, ld_c=Kb, S=7, ah=None, ld_a=0, path=3 * p, row_off=0, nrows=11, rot=4 * p, hh=5 * p, ld_h=Kb,
                P=9, k0=4, nseg=4, Kb=Kb, Ls=9, alpha=0.5, b=6 * p, ld_b=Kb)
    rows = dict(bank, w=None, ch=None, ld_c=0, S=0, ah=p, ld_a=Kb, path=None, row_off=3, nrows=5)
    for ok in (bank, rows):
        for name in ("rot", "hh", "b"):             # null pointers
            assert _compose(lib, ok, **{name: None}) == -1, name
        for name in ("P", "nseg", "Kb", "Ls", "nrows"):             # non-positive sizes
            assert _compose(lib, ok, **{name: 0}) == -1 and _compose(lib, ok, **{name: -3}) == -1, name
        assert _compose(lib, ok, k0=-1) == -1 and _compose(lib, ok, row_off=-1) == -1 and _compose(lib, ok, S=-1) == -1
        assert _compose(lib, ok, k0=6) == -1        # segments 6 .. 9 of a path of 9
        for name in ("ld_h", "ld_b"):               # pitches shorter than the row
            assert _compose(lib, ok, **{name: Kb - 1}) == -1, name
        assert _compose(lib, ok, alpha=-0.1) == -1 and _compose(lib, ok, alpha=1.5) == -1
        assert _compose(lib, ok, alpha=float("nan")) == -1
        assert _compose(lib, ok, b=6 * p + 4) == -1 and _compose(lib, ok, hh=5 * p + 4) == -1   # 8-byte aligned spectra
        assert _compose(lib, ok, rot=4 * p + 2) == -1
        assert _compose(lib, ok, Ls=17) == -2       # more than 16 channels: stock tensor operations
    assert _compose(lib, bank, w=None) == -1 and _compose(lib, bank, ch=None) == -1            # w without ch and the reverse
    assert _compose(lib, bank, ah=p) == -1          # both modes at once
    assert _compose(lib, bank, S=0) == -1           # S = 0 with w and ch
    assert _compose(lib, rows, S=3) == -1           # S > 0 without either
    assert _compose(lib, rows, ah=None) == -1       # neither mode
    assert _compose(lib, bank, ld_c=Kb - 1) == -1 and _compose(lib, rows, ld_a=Kb - 1) == -1
    assert _compose(lib, bank, ch=2 * p + 4) == -1 and _compose(lib, rows, ah=p + 4) == -1
    assert _compose(lib, bank, path=3 * p + 4) == -1
    # without a path the rows k0 - 1 - row_off .. k0 + nseg - 1 - row_off must be in the store
    assert _compose(lib, rows, row_off=4) == -1 and _compose(lib, rows, nrows=4) == -1
    assert _compose(lib, bank, S=33) == -2          # more than 32 band signals per channel: the caller renders the rows


def _ola(lib, ok, **kw):
    a = dict(ok, **kw)
    return lib.gfdn_binaural_ola(a["s"], a["ld_s"], a["nseg"], a["k0"], a["P"], a["h"], a["nb"], a["Fd"], a["tail_in"],
                                 a["tail_out"], a["out"], None)


def test_binaural_ola_argument_errors(lib):
    p = 4096
    ok = dict(s=p, ld_s=512, nseg=4, k0=4, P=9, h=48, nb=256, Fd=24, tail_in=2 * p, tail_out=3 * p, out=4 * p)
    for name in ("s", "tail_out", "out"):
        assert _ola(lib, ok, **{name: None}) == -1, name
    for name in ("nseg", "P", "h", "nb"):
        assert _ola(lib, ok, **{name: 0}) == -1 and _ola(lib, ok, **{name: -2}) == -1, name
    assert _ola(lib, ok, k0=-1) == -1
    assert _ola(lib, ok, Fd=0) == -1 and _ola(lib, ok, Fd=49) == -1          # 1 <= Fd <= h
    assert _ola(lib, ok, k0=6) == -1                # segments 6 .. 9 of a path of 9
    assert _ola(lib, ok, tail_in=None) == -1        # behind the first chunk the tail of the chunk before is needed
    assert _ola(lib, ok, tail_in=3 * p) == -1       # read and written in one launch: two buffers
    assert _ola(lib, ok, ld_s=302) == -1            # rows shorter than h + nb - 1 = 303
    assert _ola(lib, ok, P=2 ** 26, h=64) == -1     # P h >= 2^31
    assert _ola(lib, ok, out=4 * p + 4) == -1 and _ola(lib, ok, tail_out=3 * p + 4) == -1    # both ears: 8-byte accesses
