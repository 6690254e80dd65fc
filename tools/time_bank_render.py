"""Time of the full-band render of a band bank (subband.infer_bank: y = D + W C, csrc/render.hip) against the band-by-band
render it replaces (subband.infer_bands), at the headline shape: 7 octave bands, N = 16 = 4 groups x 4 lines,
nfft = 131 072 (K = 65 537), 838 synthetic receivers per band (rooms as in bench.py), 129-tap reconstructing FIRs.

One process, the same nets, datasets and taps for everything:
  infer_bands        band by band, GridLoader batches of 32 receivers: one solve, one inverse transform and one convolution
                     per receiver of every band (once: it is the slow path);
  infer_bank_first   the first call: builds the dataset constant D (every receiver's direct path through all bands);
  infer_bank         steady state: group signals of the 7 bands, gains of all receivers, the mix (median of --repeats);
  mix                the mix launch alone (device events around ``hip_ops.render_mix``), with its compulsory bytes
                     (2 R L + S L + R S) 4, the achieved GB/s and their share of the 8 TB/s HBM peak.
Prints ONE JSON line.

    python tools/time_bank_render.py [--receivers 838] [--repeats 9] [--bands 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402  (the headline workload's constants)
from time_coupled_bank import build_band  # noqa: E402  (one band of the headline recipe)

TAPS = 129
HBM_PEAK_GBS = 8000.0


def wall_ms(fn):
    """host clock around work that ends in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--receivers', type=int, default=838)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--bands', type=int, default=len(bench.BAND_CENTRES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bank_render.py measures on the GPU: no device here")
    if args.repeats < 5:
        raise SystemExit("at least 5 repeats")
    from scipy.signal import firwin
    from diffgfdn_amd import hip_ops as ops
    from diffgfdn_amd.bandbank import BandBank, BandStackedDataset
    from diffgfdn_amd.dataloader import GridLoader
    from diffgfdn_amd.subband import infer_bands, infer_bank
    device = torch.device('cuda', 0)
    centres = list(bench.BAND_CENTRES[:args.bands])
    R = args.receivers
    bands = [build_band(device, q, f, R, False) for q, f in enumerate(centres)]
    bank = BandBank([b[0] for b in bands])
    datasets = [b[1] for b in bands]
    sds = BandStackedDataset(datasets)
    nyq = bench.FS / 2
    taps = torch.tensor(np.stack([firwin(TAPS, [f / np.sqrt(2), min(f * np.sqrt(2), 0.999 * nyq)], pass_zero=False,
                                         fs=bench.FS) for f in centres]), dtype=torch.float32, device=device)

    def load_band(f):
        q = centres.index(f)
        return bank.nets[q], GridLoader(datasets[q], list(range(R)), batch_size=bench.BATCH, shuffle=False), taps[q]

    # warm-up of every kernel the band-by-band path uses (one batch of one band), then the whole render once
    infer_bands(centres[:1], lambda f: (bank.nets[0], GridLoader(datasets[0], list(range(bench.BATCH)),
                                                                 batch_size=bench.BATCH, shuffle=False), taps[0]))
    bands_ms, y_bands = wall_ms(lambda: infer_bands(centres, load_band))
    first_ms, y = wall_ms(lambda: infer_bank(bank, sds, taps))
    scale = float(y_bands.abs().max())
    parity = float((y - y_bands).abs().max()) / scale
    del y_bands
    out_buf = torch.empty_like(y)
    steady = [wall_ms(lambda: infer_bank(bank, sds, taps, out=out_buf))[0] for _ in range(args.repeats + 2)][2:]

    # the mix launch alone
    D = sds.direct_render(taps)
    C = bank.filtered_group_signals(sds.z_values, taps)
    W = bank.render_gains(sds.norm_listener_position, R)
    S, L = C.shape
    for _ in range(3):
        ops.render_mix(D, W, C, out=out_buf)
    mix = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.render_mix(D, W, C, out=out_buf)
        e1.record()
        e1.synchronize()
        mix.append(e0.elapsed_time(e1))
    mix_ms = statistics.median(mix)
    nbytes = (2 * R * L + S * L + R * S) * 4
    gbs = nbytes / (mix_ms * 1e-3) / 1e9
    out = {'what': 'full-band render of a band bank, ms', 'bands': len(centres), 'N': bench.G * bench.NPER, 'K': bench.K,
           'receivers': R, 'taps': TAPS, 'signals': S, 'samples': L, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0),
           'infer_bands_ms': round(bands_ms, 3), 'infer_bands_batch': bench.BATCH,
           'infer_bank_first_ms': round(first_ms, 3),
           'infer_bank': {'median_ms': round(statistics.median(steady), 4), 'min_ms': round(min(steady), 4),
                          'max_ms': round(max(steady), 4)},
           'infer_bands_over_infer_bank': round(bands_ms / statistics.median(steady), 2),
           'infer_bank_vs_infer_bands_rel_err': float(f"{parity:.3e}"),
           'mix': {'median_ms': round(mix_ms, 4), 'min_ms': round(min(mix), 4), 'max_ms': round(max(mix), 4),
                   'launches': (S + 31) // 32, 'compulsory_bytes': nbytes, 'flop': 2 * R * S * L,
                   'GBps': round(gbs, 1), 'fraction_of_8TBps': round(gbs / HBM_PEAK_GBS, 4),
                   'TFLOPs': round(2 * R * S * L / (mix_ms * 1e-3) / 1e12, 2)}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
