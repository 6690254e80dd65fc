"""The EDR matching error pinned to the reference: ``tests/edr_error_ref.ref_edr_error`` against
``tests/golden/f17_edr_error.npz`` (the reference's own ``get_stft_torch`` / ``get_edr_from_stft`` and plot.py:818-821 on a
seeded problem: 5 receivers, win 512, 2301 measured against 2075 estimated samples, 12 % of the measured EDR's cells on
the eps floor; ``tests/golden/gen_f17_edr_error.py``).

The reference stores the EDR in a float32 buffer before the difference, and THAT ROUNDING SHOWS: it is not a function of the
inputs alone but of the last bits of the float64 value behind it, which move with the host's FFT and log10 code -- on a
second machine one EDR cell of the fixture came out one float32 ulp (7.6e-6 dB) away.  So the fixture holds two results:
plot.py:818-821 literally (float32 buffer), which the restatement is held to by what that rounding is, and the same
reference lines with the buffer widened to float64, which it is held to at 1e-9 dB."""
import os

import numpy as np

from tests.edr_error_ref import edr_db, ref_edr_error

HERE = os.path.dirname(os.path.abspath(__file__))
# one ulp of a float32 below 128 dB: the most a cell of the reference's float32 EDR can move between two hosts
F32_ULP_128 = 2.0 ** -17


def _fixture():
    return np.load(os.path.join(HERE, "golden", "f17_edr_error.npz"))


def test_float64_restatement_equals_the_reference_lines():
    """the yardstick of the GPU tests against the reference's STFT, tail sums, dB and plot.py:818-821 with nothing
    rounded to float32: 1e-9 dB"""
    g = _fixture()
    win = int(g["win"])
    L = min(g["measured"].shape[1], g["estimated"].shape[1])
    assert g["measured"].shape[1] != g["estimated"].shape[1] and L % (win // 2) != 0
    err, rmse = ref_edr_error(g["estimated"], g["measured"], win)
    assert err.dtype == np.float64 and err.shape == g["error_db_f64"].shape
    assert float(np.abs(err - g["error_db_f64"]).max()) <= 1e-9
    assert abs(float(rmse) - float(g["rmse_f64"])) <= 1e-9
    floor = g["original_edr"].min()
    assert 0.1 < float((g["original_edr"] <= floor + 1e-3).mean()) < 0.9, "the fixture exercises the eps floor"
    assert float(g["error_db"].min()) > 1.0, "and an error of the order of dB"


def test_restatement_with_the_float32_buffer_equals_the_reference():
    """``reference_rounding=True`` restates the float32 buffer itself: every EDR cell within ONE float32 ulp of the
    reference's (0 on the machine that wrote the fixture), error_db and the rmse within the same figure (a mean of cells
    that each moved by at most one ulp, summed in float32: a few ulps of a value below 16 dB, 1e-6 dB each, on top)"""
    g = _fixture()
    win = int(g["win"])
    L = min(g["measured"].shape[1], g["estimated"].shape[1])
    for name, key in (("measured", "original_edr"), ("estimated", "est_edr")):
        got = edr_db(g[name][:, :L], win, reference_rounding=True)
        assert got.shape == g[key].shape and got.dtype == g[key].dtype == np.float32
        d = np.abs(got.astype(np.float64) - g[key])
        print(f"float32 EDR of the {name} side: {int((d > 0).sum())} of {d.size} cells differ, by at most {d.max():.3e} dB")
        assert float(d.max()) <= F32_ULP_128, name
    err, rmse = ref_edr_error(g["estimated"], g["measured"], win, reference_rounding=True)
    assert err.shape == g["error_db"].shape
    assert float(np.abs(err.astype(np.float64) - g["error_db"]).max()) <= F32_ULP_128 + 4e-6
    assert abs(float(rmse) - float(g["rmse"])) <= F32_ULP_128 + 4e-6


def test_float64_restatement_is_the_reference_up_to_its_float32_rounding():
    """The float64 yardstick differs from the reference's literal result only by the float32 EDR buffer.
    Per cell and side: the tail sum rounded to float32 (relative 2^-24: 2.6e-7 dB), the sum with eps likewise, log10 in
    float32 (about one ulp of a value below 8, times ten: 4.8e-6 dB) and the product rounded to float32 (half an ulp of a
    value below 128 dB: 3.8e-6 dB) -- under 1e-5 dB per cell and side, so under 2e-5 dB on a difference and on their mean,
    whose own float32 summation adds at most a few ulps of a value below 16 dB (1e-6 dB each).  Bound: 2.5e-5 dB."""
    g = _fixture()
    win = int(g["win"])
    err, rmse = ref_edr_error(g["estimated"], g["measured"], win)
    d = float(np.abs(err - g["error_db"].astype(np.float64)).max())
    print(f"float64 restatement against the reference's float32 EDR: error_db off by {d:.3e} dB, "
          f"rmse by {abs(float(rmse) - float(g['rmse'])):.3e} dB")
    assert d <= 2.5e-5 and abs(float(rmse) - float(g["rmse"])) <= 2.5e-5
