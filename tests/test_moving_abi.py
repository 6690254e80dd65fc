"""CPU checks of the moving-listener entry points (csrc/moving.hip): the header declares them, the built library exports them
with the argument counts of the declarations, and they report argument errors before anything is launched (there is no
device here: a launch would come back as a runtime error, not as -1)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gfdn_moving_compose", "gfdn_moving_ola")


@pytest.fixture(scope="module")
def lib():
    from diffgfdn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "diffgfdn_amd", "csrc"), "-j4"])
    return _lib.load()


def test_moving_entry_points_are_declared_and_exported(lib):
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
    return lib.gfdn_moving_compose(a["dh"], a["ld_d"], a["rows"], a["w"], a["ch"], a["ld_c"], a["xh"], a["ld_x"], a["nseg"],
                                   a["F"], a["S"], a["alpha"], a["first"], a["ema"], a["z"], a["ld_z"], None)


def test_moving_compose_argument_errors(lib):
    p = 4096                                        # any non-null address: nothing may be read or launched
    F = 257
    mixed = dict(dh=p, ld_d=F, rows=None, w=p, ch=p, ld_c=F, xh=2 * p, ld_x=F, nseg=4, F=F, S=5, alpha=0.5, first=1,
                 ema=3 * p, z=4 * p, ld_z=F)
    plain = dict(mixed, w=None, ch=None, ld_c=0, S=0)
    for ok in (mixed, plain):
        for name in ("dh", "xh", "ema", "z"):       # null pointers
            assert _compose(lib, ok, **{name: None}) == -1, name
        for name in ("nseg", "F"):                  # non-positive sizes
            assert _compose(lib, ok, **{name: 0}) == -1 and _compose(lib, ok, **{name: -3}) == -1, name
        assert _compose(lib, ok, S=-1) == -1
        for name in ("ld_d", "ld_x", "ld_z"):       # pitches shorter than the row
            assert _compose(lib, ok, **{name: F - 1}) == -1, name
        assert _compose(lib, ok, alpha=-0.1) == -1 and _compose(lib, ok, alpha=1.5) == -1
        assert _compose(lib, ok, alpha=float("nan")) == -1
        assert _compose(lib, ok, z=4 * p + 4) == -1 and _compose(lib, ok, dh=p + 4) == -1      # 8-byte aligned spectra
    assert _compose(lib, mixed, w=None) == -1 and _compose(lib, mixed, ch=None) == -1          # w without ch and the reverse
    assert _compose(lib, mixed, S=0) == -1          # S = 0 with both
    assert _compose(lib, plain, S=3) == -1          # S > 0 without either
    assert _compose(lib, mixed, ld_c=F - 1) == -1
    assert _compose(lib, mixed, S=33) == -2         # more than 32 group signals: the caller renders the rows first


def _ola(lib, ok, **kw):
    a = dict(ok, **kw)
    return lib.gfdn_moving_ola(a["s"], a["ld_s"], a["nseg"], a["k0"], a["P"], a["h"], a["Lr"], a["Fd"], a["tail_in"],
                               a["tail_out"], a["out"], None)


def test_moving_ola_argument_errors(lib):
    p = 4096
    ok = dict(s=p, ld_s=512, nseg=4, k0=4, P=9, h=48, Lr=271, Fd=24, tail_in=2 * p, tail_out=3 * p, out=4 * p)
    for name in ("s", "tail_out", "out"):
        assert _ola(lib, ok, **{name: None}) == -1, name
    for name in ("nseg", "P", "h", "Lr"):
        assert _ola(lib, ok, **{name: 0}) == -1 and _ola(lib, ok, **{name: -2}) == -1, name
    assert _ola(lib, ok, k0=-1) == -1
    assert _ola(lib, ok, Fd=0) == -1 and _ola(lib, ok, Fd=49) == -1          # 1 <= Fd <= h
    assert _ola(lib, ok, k0=6) == -1                # segments 6 .. 9 of a path of 9
    assert _ola(lib, ok, tail_in=None) == -1        # behind the first chunk the tail of the chunk before is needed
    assert _ola(lib, ok, tail_in=3 * p) == -1       # read and written in one launch: two buffers
    assert _ola(lib, ok, ld_s=317) == -1            # rows shorter than h + Lr - 1 = 318
    assert _ola(lib, ok, P=2 ** 26, h=64) == -1     # P h >= 2^31
