"""The binaural render of a moving, head-turning listener pinned to the reference: ``tests/binaural_ref.ref_binaural``
against ``tests/golden/f20_binaural.npz`` (the reference's own ``binaural_dynamic_rendering.binaural_filter_overlap_add``,
sound_examples.py:356-535, on seeded problems: fs 480, h = Fd = 48, stores of 5 ambisonic RIRs, the path
[3, 1, 1, 0, 4, 2, 3, 3, 1]; ``tests/golden/gen_f20_binaural.py``).

The reference's output is float64 and the restatement uses the same stock numpy / scipy transforms and convolution: held to
1e-12 of the largest output."""
import os

import numpy as np
import pytest

from tests.binaural_ref import fade_windows, ref_binaural, transform_length
from tests.moving_listener_ref import ms_to_samps

HERE = os.path.dirname(os.path.abspath(__file__))
NUM_CASES = 7
TOL = 1e-12


def fixture():
    return np.load(os.path.join(HERE, "golden", "f20_binaural.npz"))


def case(g, i):
    """(ambi_rirs, hrir_sh, path, rotations, stimulus, fs, update_ms, alpha, expected float64 output) of case i"""
    Ls = int(g[f"ls_{i}"])
    return (g[f"rirs_{Ls}"], g[f"{str(g[f'hrir_{i}'])}_{Ls}"], g[f"path_{i}"], g[f"rot_{i}"], g[str(g[f"stim_{i}"])],
            float(g["fs"]), float(g["update_ms"]), float(g[f"alpha_{i}"]), g[f"out_{i}"])


def test_fixture_covers_the_declared_cases():
    g = fixture()
    assert int(g["num_cases"]) == NUM_CASES
    seen = set()
    for i in range(NUM_CASES):
        rirs, hrir, path, rot, stim, fs, update_ms, alpha, out = case(g, i)
        h = ms_to_samps(update_ms, fs)
        Ls, L = rirs.shape[1], rirs.shape[2]
        assert h == 48 and out.dtype == np.float64 and out.shape == (len(path) * h, 2)
        assert rot.shape == (len(path), Ls, Ls) and hrir.shape[:2] == (Ls, 2)
        i0 = 0
        for n in (1, 3, 5)[:int(round(Ls ** 0.5))]:                 # block-orthogonal per degree
            blk = rot[:, i0:i0 + n, i0:i0 + n]
            assert np.allclose(blk @ blk.transpose(0, 2, 1), np.eye(n), atol=1e-12)
            i0 += n
        assert np.count_nonzero(rot) == len(path) * sum(n * n for n in (1, 3, 5)[:int(round(Ls ** 0.5))])
        seen.add((Ls, L, stim.size, alpha, len(path), hrir.shape[2] == transform_length(L), hrir.shape[2]))
    assert {(s[0], s[1]) for s in seen} == {(4, 200), (9, 256)}
    assert {s[2] for s in seen} == {100, 1000}, "a stimulus that is repeated and one that is cut"
    assert {s[3] for s in seen} == {0.5, 1.0, 0.25} and {s[4] for s in seen} == {9, 1}
    assert {s[5] for s in seen} == {True, False} and 24 in {s[6] for s in seen}
    assert len(set(g["path_0"].tolist())) < 9, "repeats in the path"
    # nb = 256: from k = 3 on a segment is cut at the end of the output, h + nb - 1 = 303 > 432 - 3 * 48
    assert transform_length(200) == 256 == transform_length(256) and 303 > 432 - 3 * 48 and 303 <= 432 - 2 * 48


@pytest.mark.parametrize("i", range(NUM_CASES))
def test_restatement_equals_the_reference(i):
    rirs, hrir, path, rot, stim, fs, update_ms, alpha, want = case(fixture(), i)
    got = ref_binaural(rirs, hrir, path, rot, stim, fs, update_ms, alpha)
    assert got.dtype == np.float64 and got.shape == want.shape
    big = float(np.abs(want).max())
    d = float(np.abs(got - want).max())
    print(f"[binaural golden] case {i}: off by {d:.3e}, {d / big:.2e} of the largest magnitude {big:.3f}")
    assert d <= TOL * big


def test_fades_and_scope():
    fi, fo = fade_windows(1)
    assert fi.tolist() == [0.0] and fo.tolist() == [1.0]            # linspace(-1, 1, 1) = [-1]
    fi, fo = fade_windows(48)
    assert np.allclose(fi ** 2 + fo ** 2, 1.0) and fi[0] == 0.0 and fo[-1] == 0.0
    rirs, hrir, path, rot, stim, fs, update_ms, alpha, _ = case(fixture(), 0)
    for fade_ms in (0.0, 102.5):                                    # Fd = 0 and Fd = 49 > h
        with pytest.raises(ValueError):
            ref_binaural(rirs, hrir, path, rot, stim, fs, update_ms, alpha, fade_ms)
    with pytest.raises(ValueError):                                 # HRIRs longer than nb
        ref_binaural(rirs, np.zeros((4, 2, 257)), path, rot, stim, fs, update_ms, alpha)
    with pytest.raises(ValueError):
        ref_binaural(rirs, hrir, path, rot[:-1], stim, fs, update_ms, alpha)
