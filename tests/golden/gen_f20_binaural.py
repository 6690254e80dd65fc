#!/usr/bin/env python
"""Golden vector of the binaural render of a moving, head-turning listener (f20_binaural.npz): the reference's own
``binaural_dynamic_rendering.binaural_filter_overlap_add`` (sound_examples.py:356-535) on small seeded problems.

fs = 480 Hz, update_ms = 100 (h = Fd = 48), stores of 5 ambisonic RIRs, the path [3, 1, 1, 0, 4, 2, 3, 3, 1] (P = 9,
total = 432).  Ls = 4 with L = 200 (nb = 256, n2 = 512: every segment from k = 3 on is cut at the end of the output) and
Ls = 9 with L = 256 (exactly a power of two).  Cases: a stimulus of 100 samples (repeated) and one of 1000 (cut), alpha in
{0.5, 1.0, 0.25} (the reference's driver fixes 0.5: the keyword is bound on the instance's ``get_binaural_rir``, the class
is not edited), P = 1, HRIRs of Mh = 24 samples and one set with Mh = nb.  A fresh object per case: the reference leaves
``prev_rotation_matrix`` and ``prev_ambi_rtf`` on the object.

The class is imported unmodified.  Stand-ins, in this generator only: the room is an object with the attributes the class
reads (``late_rirs`` is the path's RIRs in order: the reference indexes its store by the segment number, and its
constructor always takes the late RIRs; ``early_late_split`` does nothing); the HRTF reader hands out the case's SH-domain
HRIRs; ``sound_examples.spa`` is a namespace whose ``sph.sh_rotation_matrix`` hands out the case's seeded matrices in call
order (spaudiopy is absent here; block-orthogonal per degree, blocks of 1, 3, 5).  The arrays are stored as float32 and
handed to the reference as the float64 of those values.  Run from the repository root where the reference sources are
present:

    python tests/golden/gen_f20_binaural.py
"""
import functools
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.install()
for _name in ("pyloudnorm", "sofa_parser"):
    if _name not in sys.modules and importlib.util.find_spec(_name) is None:
        _m = types.ModuleType(_name)
        _m.HRIRSOFAReader = object
        sys.modules[_name] = _m
for _name in ("spatial_sampling.dataloader", "diff_gfdn.dataloader"):
    # (only the class names are imported, for annotations; the real modules pull in packages that are absent here)
    try:
        importlib.import_module(_name)
    except Exception:                                              # noqa: BLE001
        _m = types.ModuleType(_name)
        _m.SpatialRoomDataset = _m.RoomDataset = object
        sys.modules[_name] = _m
import sound_examples  # noqa: E402
from sound_examples import binaural_dynamic_rendering  # noqa: E402

FS, UPDATE_MS, R = 480.0, 100.0, 5
PATH = [3, 1, 1, 0, 4, 2, 3, 3, 1]
SIZES = {4: 200, 9: 256}                                           # Ls -> L
# (Ls, stimulus, path, alpha, hrir set)
CASES = [(4, "s100", PATH, 0.5, "h24"), (4, "s1000", PATH, 1.0, "h24"), (4, "s1000", PATH, 0.25, "h24"),
         (9, "s100", PATH, 0.5, "h24"), (9, "s1000", PATH, 0.25, "h24"), (4, "s100", [3], 0.5, "h24"),
         (4, "s100", PATH, 0.5, "hnb")]


class Room:
    """what ``binaural_dynamic_rendering`` reads of a SpatialRoomDataset"""

    def __init__(self, rirs, order):
        self.rirs, self.late_rirs, self.sample_rate = rirs, rirs.copy(), FS
        self.ambi_order, self.rir_length = order, rirs.shape[-1]
        self.num_rooms, self.room_dims, self.room_start_coord, self.aperture_coords = 1, [(4.0, 5.0, 3.0)], [(0.0, 0.0, 0.0)], []

    def early_late_split(self, win_len_ms=10):
        pass


class Reader:
    """what it reads of an HRIRSOFAReader"""

    def __init__(self, hrir_sh):
        self.fs, self.hrir_sh = FS, hrir_sh

    def get_spherical_harmonic_representation(self, order):
        assert self.hrir_sh.shape[0] == (order + 1) ** 2
        return self.hrir_sh


def rotation(rng, Ls):
    """block-orthogonal per degree"""
    out, i, deg = np.zeros((Ls, Ls)), 0, 0
    while i < Ls:
        n = 2 * deg + 1
        out[i:i + n, i:i + n] = np.linalg.qr(rng.randn(n, n))[0]
        i, deg = i + n, deg + 1
    return out


def main():
    rng = np.random.RandomState(20)
    f32 = lambda a: a.astype(np.float32)                           # noqa: E731
    save = dict(fs=np.float64(FS), update_ms=np.float64(UPDATE_MS), num_cases=np.int64(len(CASES)),
                s100=f32(rng.randn(100)), s1000=f32(rng.randn(1000)))
    for Ls, L in SIZES.items():
        env = np.exp(-np.arange(L) / 50.0)
        save[f"rirs_{Ls}"] = f32(env * rng.randn(R, Ls, L))
        nb = 2 ** int(np.ceil(np.log2(L)))
        save[f"h24_{Ls}"] = f32(rng.randn(Ls, 2, 24) * np.exp(-np.arange(24) / 6.0))
        save[f"hnb_{Ls}"] = f32(rng.randn(Ls, 2, nb) * np.exp(-np.arange(nb) / 40.0))
    for i, (Ls, stim, path, alpha, hset) in enumerate(CASES):
        P, order = len(path), int(round(Ls ** 0.5)) - 1
        rots = np.stack([rotation(rng, Ls) for _ in path])
        queue = list(rots)
        sound_examples.spa = types.SimpleNamespace(sph=types.SimpleNamespace(
            sh_rotation_matrix=lambda *a, **k: queue.pop(0)))
        rirs = save[f"rirs_{Ls}"].astype(np.float64)[path]
        pos = np.array([[float(p), 0.0, 0.0] for p in path])
        orient = rng.uniform(-1.0, 1.0, size=(P, 2))
        obj = binaural_dynamic_rendering(Room(rirs, order), pos, orient, save[stim].astype(np.float64),
                                         Reader(save[f"{hset}_{Ls}"].astype(np.float64)), update_ms=UPDATE_MS)
        obj.get_binaural_rir = functools.partial(obj.get_binaural_rir, alpha=alpha)
        out = obj.binaural_filter_overlap_add()
        assert not queue and out.dtype == np.float64 and out.shape == (P * obj.hop_size, 2)
        save.update({f"ls_{i}": np.int64(Ls), f"stim_{i}": np.array(stim), f"path_{i}": np.array(path, dtype=np.int64),
                     f"alpha_{i}": np.float64(alpha), f"hrir_{i}": np.array(hset), f"rot_{i}": rots, f"out_{i}": out})
        print(f"case {i}: Ls {Ls}, {stim}, P = {P}, alpha {alpha}, {hset}: |out| <= {np.abs(out).max():.3f}")
    np.savez_compressed(os.path.join(HERE, "f20_binaural.npz"), **save)


if __name__ == "__main__":
    main()
