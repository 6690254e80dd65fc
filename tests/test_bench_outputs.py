"""bench.py --dump-outputs: the host side of it (what is written, in which precision, under which size bound)."""
import os

import numpy as np
import torch

import bench


def _collected():
    arrays = {}
    parts = {'_total': torch.arange(7, dtype=torch.float32), 'edr_loss': torch.ones(7, dtype=torch.float64),
             'spectrum': torch.ones(3, dtype=torch.complex64), 'steps': 3}
    bench.collect_outputs('loss', parts, arrays)
    net = torch.nn.Linear(3, 4)

    class Opt:
        flat_grad = torch.full((16,), 0.5)
    bench.collect_model(net, Opt(), arrays)
    return parts, arrays


def test_collected_outputs_are_host_copies_in_float32_or_float64():
    parts, arrays = _collected()
    assert set(arrays) == {'loss_total', 'loss_edr_loss', 'loss_spectrum', 'loss_steps', 'param_weight', 'param_bias',
                           'grad_flat'}
    assert arrays['loss_total'].dtype == np.float32 and arrays['loss_edr_loss'].dtype == np.float64
    assert arrays['loss_spectrum'].shape == (3, 2) and arrays['loss_spectrum'].dtype == np.float32
    parts['_total'].zero_()                      # (the step's loss tensors are static buffers: the dump must not alias them)
    assert arrays['loss_total'].tolist() == list(range(7))


def test_dump_keeps_small_arrays_whole_and_samples_large_ones_reproducibly(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 4096)
    big = np.arange(5000, dtype=np.float32)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'small': np.arange(5, dtype=np.float64), 'big': big.copy()})
    a = {f: np.load(tmp_path / 'a' / f) for f in sorted(os.listdir(tmp_path / 'a'))}
    b = {f: np.load(tmp_path / 'b' / f) for f in sorted(os.listdir(tmp_path / 'b'))}
    assert list(a) == ['big.npy', 'small.npy']
    assert sum(v.nbytes for v in a.values()) <= 4096
    assert a['small.npy'].tolist() == [0, 1, 2, 3, 4]
    assert a['big.npy'].size == 2048 // 4 and np.all(np.diff(a['big.npy']) > 0)      # a sorted sample of the flat array
    assert all(np.array_equal(a[f], b[f]) for f in a)
