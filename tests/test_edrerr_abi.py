"""CPU checks of the EDR-error entry points (csrc/edrerr.hip, gfdn_stft_spectrum in csrc/fft.hip): the library exports them
and they report argument errors before anything is launched (there is no device here: a launch would come back as a
runtime error, not as -1)."""
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


def test_edr_err_is_exported(lib):
    from diffgfdn_amd import _lib
    for name in ("gfdn_edr_err", "gfdn_edr_err_work_bytes", "gfdn_stft_spectrum"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.gfdn_abi_version() == _lib.ABI_VERSION == 8          # purely additive
    assert lib.gfdn_edr_err_work_bytes(838, 2049) == 838 * 33 * 8   # one float64 per receiver and tile of 64 bins
    assert lib.gfdn_edr_err_work_bytes(0, 5) == 0


def _call(lib, ok, **kw):
    a = dict(ok, **kw)
    return lib.gfdn_edr_err(a["sd"], a["ld_d"], a["rows"], a["w"], a["sc"], a["ld_c"], a["tdb"], a["ld_t"], a["R"], a["T"],
                            a["F"], a["S"], a["mode"], a["out"], a["ld_o"], a["work"], None)


def test_edr_err_argument_errors(lib):
    p = 4096                                        # any non-null address: nothing may be read or launched
    R, T, F, S = 3, 4, 100, 5
    err = dict(sd=p, ld_d=F, rows=None, w=p, sc=p, ld_c=F, tdb=p, ld_t=F, R=R, T=T, F=F, S=S, mode=0, out=2 * p, ld_o=0,
               work=3 * p)
    curve = dict(err, tdb=None, ld_t=0, mode=1, ld_o=F, work=None)
    for ok in (err, curve):
        for name in ("sd", "out"):                  # null pointers
            assert _call(lib, ok, **{name: None}) == -1, name
        for name in ("R", "T", "F"):                # non-positive sizes
            assert _call(lib, ok, **{name: 0}) == -1 and _call(lib, ok, **{name: -3}) == -1, name
        assert _call(lib, ok, S=-1) == -1
        assert _call(lib, ok, ld_d=F - 1) == -1 and _call(lib, ok, ld_c=F - 1) == -1      # pitches shorter than the row
        assert _call(lib, ok, w=None) == -1 and _call(lib, ok, sc=None) == -1             # w without sc and the reverse
        assert _call(lib, ok, w=None, sc=None) == -1                                      # S > 0 without either
        assert _call(lib, ok, S=0) == -1                                                  # S = 0 with both
        assert _call(lib, ok, S=33) == -2           # more than 32 group signals per launch: the caller mixes them first
        assert _call(lib, ok, mode=2) == -1 and _call(lib, ok, mode=-1) == -1
    assert _call(lib, err, tdb=None) == -1
    assert _call(lib, err, ld_t=F - 1) == -1
    assert _call(lib, err, work=None) == -1 and _call(lib, err, work=3 * p + 4) == -1     # the float64 partial sums
    assert _call(lib, curve, ld_o=F - 1) == -1      # curve (R, T, ld_o): rows shorter than F


def test_stft_spectrum_argument_errors(lib):
    p = 4096
    ok = dict(x=p, ld=3000, T=3000, L=3000, batch=2, win=512, S=2 * p, ld_f=257)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gfdn_stft_spectrum(a["x"], a["ld"], a["T"], a["L"], a["batch"], a["win"], a["S"], a["ld_f"], None)
    assert call(x=None) == -1 and call(S=None) == -1 and call(S=2 * p + 4) == -1
    assert call(batch=0) == -1 and call(T=0) == -1
    assert call(T=3001) == -1                       # more valid samples than the length that defines the frames
    assert call(ld=2999) == -1 and call(ld_f=256) == -1
    assert call(win=500) == -1                      # not a power of two
    assert call(T=100, L=100, ld=100) == -1         # ceil(L / hop) hop < win: no frame
    assert call(batch=65536) == -2
