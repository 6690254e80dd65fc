"""The moving-listener render pinned to the reference: ``tests/moving_listener_ref.ref_moving_listener`` against
``tests/golden/f18_moving_listener.npz`` (the reference's own ``filter_overlap_add``, sound_examples.py:163-226, on a seeded
problem: fs 480, h = 48, 11 RIRs of 271 samples, path [3, 7, 7, 0, 10, 2, 5, 5, 1]; ``tests/golden/gen_f18_moving_listener.py``).

The reference accumulates its float64 segments into a FLOAT32 output: every ``+=`` rounds the running sum.  A sample is
covered by at most ceil((h + Lr - 1) / h) = 7 segments and each rounding moves it by at most half an ulp of the running sum,
which is of the size of the output: the float64 restatement is held to 7 x 0.5 = 3.5 float32 ulps of the output's largest
magnitude.  Measured over the nine cases: 0.48 .. 1.37 ulps."""
import os

import numpy as np
import pytest

from tests.moving_listener_ref import extended_stimulus, ms_to_samps, overlap_add, ref_moving_listener, segments

HERE = os.path.dirname(os.path.abspath(__file__))
ULPS = 3.5


def fixture():
    return np.load(os.path.join(HERE, "golden", "f18_moving_listener.npz"))


def case(g, i):
    """(rirs, path, stimulus, fs, update_ms, alpha, fade_len_ms, expected float32 output) of case i"""
    rirs = g["rirs"] if bool(g[f"whole_{i}"]) else g["late_rirs"]
    return (rirs, g[f"path_{i}"], g[str(g[f"stim_{i}"])], float(g["fs"]), float(g["update_ms"]), float(g[f"alpha_{i}"]),
            float(g[f"fade_len_ms_{i}"]), g[f"out_{i}"])


NUM_CASES = 9


def test_fixture_covers_the_declared_cases():
    g = fixture()
    assert int(g["num_cases"]) == NUM_CASES and g["rirs"].shape == g["late_rirs"].shape == (11, 271)
    seen = set()
    for i in range(NUM_CASES):
        rirs, path, stim, fs, update_ms, alpha, fade_ms, out = case(g, i)
        h, Fd = ms_to_samps(update_ms, fs), ms_to_samps(fade_ms, fs)
        assert h == 48 and out.dtype == np.float32 and out.shape == (len(path) * h,)
        seen.add((stim.size, alpha, Fd, len(path), bool(g[f"whole_{i}"])))
    assert {s[0] for s in seen} == {100, 1000}, "a stimulus that is repeated and one that is cut"
    assert {s[1] for s in seen} == {0.5, 1.0, 0.25} and {s[2] for s in seen} == {24, 48, 1}
    assert {s[3] for s in seen} == {9, 1} and {s[4] for s in seen} == {True, False}
    # from k = 3 on a segment is cut at the end of the output: h + Lr - 1 = 318 > 432 - 3 * 48
    assert 48 + 271 - 1 > 432 - 3 * 48 and 48 + 271 - 1 <= 432 - 2 * 48


@pytest.mark.parametrize("i", range(NUM_CASES))
def test_restatement_equals_the_reference(i):
    rirs, path, stim, fs, update_ms, alpha, fade_ms, want = case(fixture(), i)
    got = ref_moving_listener(rirs, path, stim, fs, update_ms, alpha, fade_ms)
    assert got.dtype == np.float64 and got.shape == want.shape
    big = float(np.abs(want).max())
    ulp = float(np.spacing(np.float32(big)))
    d = float(np.abs(got - want.astype(np.float64)).max())
    print(f"[moving golden] case {i}: off by {d:.3e} = {d / ulp:.2f} float32 ulps of the largest magnitude {big:.3f}")
    assert d <= ULPS * ulp


@pytest.mark.parametrize("i", range(NUM_CASES))
def test_identity_form_equals_the_branchy_form(i):
    """out = OLA(s) + fade_out (t - s) on the faded samples is the reference's own loop (fade_in + fade_out = 1): both in
    float64 on the same segments, they differ by a few float64 roundings"""
    rirs, path, stim, fs, update_ms, alpha, fade_ms, want = case(fixture(), i)
    h, Fd = ms_to_samps(update_ms, fs), ms_to_samps(fade_ms, fs)
    segs = segments(rirs, [int(p) for p in path], extended_stimulus(stim, len(path) * h), h, alpha)
    a, b = overlap_add(segs, h, Fd), overlap_add(segs, h, Fd, branchy=True)
    assert float(np.abs(a - b).max()) <= 1e-13 * float(np.abs(b).max())
    for k, s in enumerate(segs):
        assert s.size == min(h + rirs.shape[1] - 1, len(path) * h - k * h) >= Fd


def test_out_of_scope_fades_raise():
    rirs, path, stim, fs, update_ms, alpha, _, _ = case(fixture(), 0)
    for fade_ms in (0.0, 102.5):                                    # Fd = 0 and Fd = 49 > h
        with pytest.raises(ValueError):
            ref_moving_listener(rirs, path, stim, fs, update_ms, alpha, fade_ms)
