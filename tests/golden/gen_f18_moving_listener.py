#!/usr/bin/env python
"""Golden vector of the moving-listener render (f18_moving_listener.npz): the reference's own
``dynamic_rendering_moving_receiver.filter_overlap_add`` (sound_examples.py:163-226) on a small seeded problem.

fs = 480 Hz, update_ms = 100 (h = 48), 11 RIRs of 271 samples (and 11 "late" ones), the path [3, 7, 7, 0, 10, 2, 5, 5, 1]
(P = 9, total = 432): every segment from k = 3 on is cut at the end of the output, which puts its cross-fade tail in the
middle of the RIR.  Cases: a stimulus of 100 samples (repeated) and one of 1000 (cut), alpha in {0.5, 1.0, 0.25},
Fd = 24, Fd = h, Fd = 1, P = 1, use_whole_rir true and false.  A fresh object per case: the reference leaves
``prev_filter`` on the object between calls.

The class is imported unmodified; the room is a stand-in object with the attributes it reads.  ``pyloudnorm`` and
``sofa_parser`` are imported by the module and used by none of the lines run here: absent, they get empty stand-ins, in this
generator only.  Run from the repository root where the reference sources are present:

    python tests/golden/gen_f18_moving_listener.py
"""
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
from sound_examples import dynamic_rendering_moving_receiver  # noqa: E402

FS, UPDATE_MS, R, LR = 480.0, 100.0, 11, 271
PATH = [3, 7, 7, 0, 10, 2, 5, 5, 1]
# (stimulus, path, alpha, fade_len_ms, use_whole_rir); 2.5 ms is one sample, 100 ms the whole update interval
CASES = [("s100", PATH, 0.5, 50.0, True), ("s1000", PATH, 0.5, 50.0, True), ("s100", PATH, 1.0, 50.0, True),
         ("s1000", PATH, 0.25, 50.0, True), ("s100", PATH, 0.5, 100.0, True), ("s1000", PATH, 0.5, 2.5, True),
         ("s100", [3], 0.5, 50.0, True), ("s1000", PATH, 0.5, 50.0, False), ("s100", PATH, 0.25, 100.0, False)]


class Room:
    """what ``dynamic_rendering_moving_receiver`` reads of a RoomDataset"""

    def __init__(self, rirs, late_rirs):
        self.rirs, self.late_rirs, self.sample_rate = rirs, late_rirs, FS
        self.num_rooms, self.room_dims, self.room_start_coord, self.aperture_coords = 1, [(4.0, 5.0, 3.0)], [(0.0, 0.0, 0.0)], []

    @staticmethod
    def find_rec_idx_in_room_dataset(rec_pos_list):
        return [int(p[0]) for p in rec_pos_list]                   # (the stand-in positions carry their row)


def main():
    rng = np.random.RandomState(18)
    env = np.exp(-np.arange(LR) / 60.0)
    rirs = env * rng.randn(R, LR)
    late = rirs * (1.0 - np.exp(-np.arange(LR) / 15.0)) + 0.05 * env * rng.randn(R, LR)
    stims = {"s100": rng.randn(100), "s1000": rng.randn(1000)}
    save = dict(rirs=rirs, late_rirs=late, fs=np.float64(FS), update_ms=np.float64(UPDATE_MS), num_cases=np.int64(len(CASES)),
                **stims)
    for i, (stim, path, alpha, fade_ms, whole) in enumerate(CASES):
        pos = np.array([[float(p), 0.0, 0.0] for p in path])
        obj = dynamic_rendering_moving_receiver(Room(rirs.copy(), late.copy()), pos, stims[stim], update_ms=UPDATE_MS)
        out = obj.filter_overlap_add(use_whole_rir=whole, alpha=alpha, fade_len_ms=fade_ms)
        assert out.dtype == np.float32 and out.shape == (len(path) * obj.hop_size,)
        save.update({f"stim_{i}": np.array(stim), f"path_{i}": np.array(path, dtype=np.int64), f"alpha_{i}": np.float64(alpha),
                     f"fade_len_ms_{i}": np.float64(fade_ms), f"whole_{i}": np.bool_(whole), f"out_{i}": out})
        print(f"case {i}: {stim}, P = {len(path)}, alpha {alpha}, fade {fade_ms} ms, whole {whole}: "
              f"|out| <= {np.abs(out).max():.3f}")
    np.savez_compressed(os.path.join(HERE, "f18_moving_listener.npz"), **save)


if __name__ == "__main__":
    main()
