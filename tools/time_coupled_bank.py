"""Step time of a band bank with learnable inter-group coupling (run_subband_training_treble.py --allow_coupling) against
what the bands cost one by one, at the headline shape: 7 octave bands, N = 16 = 4 groups x 4 lines, nfft = 131 072
(K = 65 537), 32 receivers per band and step, synthetic rooms as in bench.py.

Three graph-replayed steps, every one normalize + forward + losses + backward + Adam:
  coupled_bank       one BandBank of 7 coupled bands (autograd path: coupled matrices of all bands in one launch, per-bin
                     elimination with the bands as blocks of 16 lines);
  zero_bank_autograd the zero-coupling bank held to the same autograd path (use_fused = False: per-bin elimination on 28
                     blocks of 4 lines) -- what coupling costs on that path;
  coupled_bands      seven single-band coupled VarReceiverPosTrainer steps replayed back to back -- what a user of coupled
                     bands had before the bank took them.
One warm-up round, then ``--repeats`` rounds of ``--replays`` replays per configuration, the configurations taking turns
inside every round; every step fetches its receivers from a schedule on the device.  Prints ONE JSON line: per
configuration the median, smallest and largest ms per step over the rounds.

    python tools/time_coupled_bank.py [--receivers 64] [--repeats 7] [--replays 20] [--bands 7]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the headline workload's constants, filters and trainer settings)


def build_band(device, q, centre_hz, receivers, coupled):
    """(net, dataset, filter) of one band: bench.build_workload's recipe with the coupling switched"""
    from diffgfdn_amd.config import CouplingMatrixType, DiffGFDNConfig, FeedbackLoopConfig, OutputFilterConfig
    from diffgfdn_amd.dataloader import MultiRIRDataset, RoomDataset
    from diffgfdn_amd.model import DiffGFDNVarReceiverPos
    from diffgfdn_amd.synthetic import synthetic_room
    room = synthetic_room(receivers, bench.G, bench.FS, 64000, seed=q, t60_range=(0.3, 1.5))
    data = MultiRIRDataset(device, RoomDataset(bench.G, bench.FS, room['source_position'], room['receiver_position'],
                                               room['rirs'], room['common_decay_times'], nfft=bench.NFFT, device=device))
    torch.manual_seed(1234 + q)
    np.random.seed(1234 + q)
    delays = DiffGFDNConfig(num_groups=bench.G, num_delay_lines=bench.G * bench.NPER, sample_rate=bench.FS,
                            seed=23463 + int(centre_hz)).delay_length_samps
    fl = FeedbackLoopConfig(coupling_matrix_type=CouplingMatrixType.SCALAR, use_zero_coupling=not coupled)
    hidden, neurons = bench.recipe_network(centre_hz)
    of = OutputFilterConfig(use_svfs=False, num_hidden_layers=hidden, num_neurons_per_layer=neurons,
                            num_fourier_features=20)
    net = DiffGFDNVarReceiverPos(bench.FS, bench.G, delays, device, fl, of, use_absorption_filters=False,
                                 common_decay_times=room['common_decay_times'], use_colorless_loss=True).to(device)
    filt = torch.tensor(bench.octave_band_response(centre_hz, bench.FS, bench.NFFT), device=device).to(torch.complex64)
    return net, data, filt


def bank_step(device, centres, receivers, coupled, use_fused):
    from diffgfdn_amd.bandbank import BandBank, BandBankTrainer, BandStackedDataset
    bands = [build_band(device, q, f, receivers, coupled) for q, f in enumerate(centres)]
    bank = BandBank([b[0] for b in bands])
    BandBankTrainer.use_fused = use_fused
    try:
        tr = BandBankTrainer(bank, bench.trainer_config(500.0, 1), subband_filter_freq_resp=torch.stack([b[2] for b in bands]),
                             band_names=[int(f) for f in centres])
    finally:
        BandBankTrainer.use_fused = True
    assert tr._fused is None, "the timed bank steps are the autograd path's"
    sds = BandStackedDataset([b[1] for b in bands], free_sources=True)
    step = tr.graphed(sds, bench.BATCH, mask_seed=7)
    rng = np.random.RandomState(5)
    sched = [sds.global_rows([rng.choice(receivers, bench.BATCH, replace=False).tolist() for _ in centres]) for _ in range(8)]
    step.capture(sched[0])
    step.load_schedule(sched)
    return [step]


def band_steps(device, centres, receivers):
    from diffgfdn_amd.trainer import VarReceiverPosTrainer
    steps = []
    rng = np.random.RandomState(5)
    for q, f in enumerate(centres):
        net, data, filt = build_band(device, q, f, receivers, True)
        tr = VarReceiverPosTrainer(net, bench.trainer_config(f, 1), subband_filter_freq_resp=filt, capturable=True)
        step = tr.graphed(data, bench.BATCH, mask_seed=7)
        sched = [rng.choice(receivers, bench.BATCH, replace=False).tolist() for _ in range(8)]
        step.capture(sched[0])
        step.load_schedule(sched)
        steps.append(step)
    return steps


def timed(steps, replays):
    """ms per step: ``replays`` times every graph of the configuration, between two device synchronisations"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        for s in steps:
            s.run_next()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / replays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--receivers', type=int, default=64, help='receivers per band in the datasets (32 of them per step)')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--replays', type=int, default=20)
    ap.add_argument('--bands', type=int, default=len(bench.BAND_CENTRES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_coupled_bank.py measures on the GPU: no device here")
    if args.repeats < 5 or args.receivers < bench.BATCH:
        raise SystemExit("at least 5 repeats and 32 receivers per band")
    warnings.filterwarnings("ignore", message="BandBankTrainer: this layout", category=RuntimeWarning)
    device = torch.device('cuda', 0)
    centres = bench.BAND_CENTRES[:args.bands]
    configs = {'coupled_bank': bank_step(device, centres, args.receivers, True, True),
               'zero_bank_autograd': bank_step(device, centres, args.receivers, False, False),
               'coupled_bands': band_steps(device, centres, args.receivers)}
    for steps in configs.values():                      # warm-up round
        timed(steps, args.replays)
    ms = {k: [] for k in configs}
    for _ in range(args.repeats):
        for k, steps in configs.items():
            ms[k].append(timed(steps, args.replays))
    out = {'what': 'ms per optimiser step of all bands, graph replay', 'bands': len(centres), 'N': bench.G * bench.NPER,
           'K': bench.K, 'receivers_per_band_and_step': bench.BATCH, 'repeats': args.repeats, 'replays': args.replays,
           'device': torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        out[k] = {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4)}
    out['coupled_bank_over_coupled_bands'] = round(out['coupled_bank']['median_ms'] / out['coupled_bands']['median_ms'], 4)
    out['coupled_bank_over_zero_bank_autograd'] = round(out['coupled_bank']['median_ms']
                                                        / out['zero_bank_autograd']['median_ms'], 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
