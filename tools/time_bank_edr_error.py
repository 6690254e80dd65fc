"""Time of the EDR matching error of a band bank's render (subband.edr_error_bank, csrc/edrerr.hip) against the path a user
had before it, at the headline shape: 7 octave bands, N = 16 = 4 groups x 4 lines, nfft = 131 072 (K = 65 537), 838
synthetic receivers per band (rooms as in bench.py), 129-tap FIRs, synthetic measured RIRs of 64 000 samples (decaying
noise), win 4096 / hop 2048: L = 64 000 samples, 31 frames of 2049 bins.

One process, the same bank, dataset, taps and measured RIRs for everything; medians of --repeats with the min - max range:
  by_hand          infer_bank -> hip_ops.stft_power in chunks of 32 receivers -> hip_ops.edr_target (tail sums and dB) ->
                   torch |difference| / mean, with the measured side's EDR precomputed (so that only the estimate's work
                   is compared);
  bank_first       edr_error_bank, first call: builds the dataset constants Sd and Tdb;
  bank             edr_error_bank, steady state;
  kernel           the launch alone (device events around ``hip_ops.edr_error``), with its compulsory bytes
                   R T F (8 + 4) + S T F 8 -- Sd and Tdb once, Sc once -- the achieved TB/s and their share of the 8 TB/s
                   HBM peak.
Prints ONE JSON line (kept as profiles/r13_bank_edr_error.json).

    python tools/time_bank_edr_error.py [--receivers 838] [--repeats 9] [--bands 7] [--samples 64000]
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
WIN = 4096
HBM_PEAK_GBS = 8000.0


def wall_ms(fn):
    """host clock around work that ends in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--receivers', type=int, default=838)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--bands', type=int, default=len(bench.BAND_CENTRES))
    ap.add_argument('--samples', type=int, default=64000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bank_edr_error.py measures on the GPU: no device here")
    if args.repeats < 5:
        raise SystemExit("at least 5 repeats")
    from scipy.signal import firwin
    from diffgfdn_amd import hip_ops as ops
    from diffgfdn_amd.bandbank import BandBank, BandStackedDataset
    from diffgfdn_amd.subband import edr_error_bank, infer_bank
    device = torch.device('cuda', 0)
    centres = list(bench.BAND_CENTRES[:args.bands])
    R = args.receivers
    bands = [build_band(device, q, f, R, False) for q, f in enumerate(centres)]
    bank = BandBank([b[0] for b in bands])
    sds = BandStackedDataset([b[1] for b in bands])
    nyq = bench.FS / 2
    taps = torch.tensor(np.stack([firwin(TAPS, [f / np.sqrt(2), min(f * np.sqrt(2), 0.999 * nyq)], pass_zero=False,
                                         fs=bench.FS) for f in centres]), dtype=torch.float32, device=device)
    nfft = 2 * (bench.K - 1)
    Tx = args.samples
    gen = torch.Generator(device=device).manual_seed(13)
    t = torch.arange(Tx, device=device, dtype=torch.float32)
    measured = 0.05 * torch.exp(-t / (0.15 * bench.FS)) * torch.randn((R, Tx), generator=gen, device=device)
    L = min(Tx, nfft + TAPS - 1)
    F = WIN // 2 + 1
    T = ops.stft_nframes(L, WIN)

    # ---- the path by hand; the measured side's EDR precomputed, outside the dataset's cache
    Tdb_hand = torch.empty((R, T, F), dtype=torch.float32, device=device)
    for r0 in range(0, R, 32):
        Tdb_hand[r0:r0 + 32] = ops.edr_target(ops.stft_power(measured[r0:r0 + 32, :L], WIN))[0]

    def by_hand():
        y = infer_bank(bank, sds, taps)
        err = torch.empty((R,), dtype=torch.float32, device=device)
        for r0 in range(0, R, 32):
            edr = ops.edr_target(ops.stft_power(y[r0:r0 + 32, :L], WIN))[0]
            err[r0:r0 + 32] = (edr - Tdb_hand[r0:r0 + 32]).abs().mean(dim=(1, 2))
        return err, torch.linalg.vector_norm(err) / R ** 0.5

    by_hand()
    hand = [wall_ms(by_hand) for _ in range(args.repeats)]
    err_hand = hand[-1][1][0].clone()
    hand = [h[0] for h in hand]
    del Tdb_hand
    torch.cuda.empty_cache()

    # ---- the bank's call
    first_ms, (err, rmse) = wall_ms(lambda: edr_error_bank(bank, sds, taps, measured))
    steady = [wall_ms(lambda: edr_error_bank(bank, sds, taps, measured))[0] for _ in range(args.repeats + 2)][2:]
    parity = float((err - err_hand).abs().max())

    # ---- the launch alone
    Sd = sds.direct_render_stft(taps, L, WIN)
    Tdb = sds.edr_error_target(measured, L, WIN)
    Sc = bank.stft_group_signals(sds.z_values, taps, L, WIN)
    W = bank.render_gains(sds.norm_listener_position, R)
    S = W.shape[1]
    out = torch.empty((R,), dtype=torch.float32, device=device)
    for _ in range(3):
        ops.edr_error(Sd, Tdb, W=W, Sc=Sc, out=out)
    kern = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.edr_error(Sd, Tdb, W=W, Sc=Sc, out=out)
        e1.record()
        e1.synchronize()
        kern.append(e0.elapsed_time(e1))
    k_ms = statistics.median(kern)
    nbytes = R * T * F * 12 + S * T * F * 8
    gbs = nbytes / (k_ms * 1e-3) / 1e9
    res = {'what': 'EDR matching error of a band bank over the receiver grid, ms', 'bands': len(centres),
           'N': bench.G * bench.NPER, 'K': bench.K, 'receivers': R, 'taps': TAPS, 'signals': S, 'samples': L, 'win': WIN,
           'frames': T, 'bins': F, 'repeats': args.repeats, 'device': torch.cuda.get_device_name(0),
           'Sd_bytes': R * T * int(Sd.stride(1)) * 8, 'Tdb_bytes': R * T * int(Tdb.stride(1)) * 4,
           'by_hand': stats(hand), 'bank_first_ms': round(first_ms, 3), 'bank': stats(steady),
           'by_hand_over_bank': round(statistics.median(hand) / statistics.median(steady), 2),
           'bank_below_by_hand': max(steady) < min(hand),
           'bank_vs_by_hand_max_abs_dB': float(f"{parity:.3e}"), 'rmse_dB': round(float(rmse), 4),
           'kernel': dict(stats(kern), compulsory_bytes=nbytes, TBps=round(gbs / 1e3, 3),
                          fraction_of_8TBps=round(gbs / HBM_PEAK_GBS, 4), fma=2 * R * S * T * F)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
