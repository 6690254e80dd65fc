"""Time of the EDC matching error of a band bank's render (subband.edc_error_bank, csrc/edcerr.hip) against the path a user
had before it, at the headline shape: 7 octave bands, N = 16 = 4 groups x 4 lines, nfft = 131 072 (K = 65 537), 838
synthetic receivers per band (rooms as in bench.py), 129-tap FIRs (reconstruction and analysis), synthetic measured RIRs
of the transform's length (decaying noise), L = min(Tx, Ty, 2 fs) samples per band signal.

One process, the same bank, dataset, taps and measured RIRs for everything; medians of --repeats with the min - max range:
  by_hand          infer_bank -> band_split of the estimate -> torch flip / cumsum / log10 / |difference| / mean, with the
                   measured side's dB curves precomputed (so that only the estimate's work is compared);
  bank_first       edc_error_bank, first call: builds the dataset constants Dk and Tdb;
  bank             edc_error_bank, steady state;
  kernel           the launch alone (device events around ``hip_ops.edc_error``), with its compulsory bytes
                   (2 R A L + A S L) 4 -- Dk and Tdb once, Ck once -- the achieved TB/s and their share of the 8 TB/s HBM peak.
Prints ONE JSON line (kept as profiles/r11_bank_edc_error.json).

    python tools/time_bank_edc_error.py [--receivers 838] [--repeats 9] [--bands 7]
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
EPS = float(np.finfo(np.float32).eps)


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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bank_edc_error.py measures on the GPU: no device here")
    if args.repeats < 5:
        raise SystemExit("at least 5 repeats")
    from scipy.signal import firwin
    from diffgfdn_amd import hip_ops as ops
    from diffgfdn_amd.bandbank import BandBank, BandStackedDataset
    from diffgfdn_amd.subband import band_split, edc_error_bank, infer_bank
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
    gen = torch.Generator(device=device).manual_seed(11)
    t = torch.arange(nfft, device=device, dtype=torch.float32)
    measured = 0.05 * torch.exp(-t / (0.15 * bench.FS)) * torch.randn((R, nfft), generator=gen, device=device)
    L = min(nfft, nfft + TAPS - 1, int(2 * bench.FS))
    A = taps.shape[0]

    # ---- the path by hand; the measured side's curves precomputed, outside the dataset's cache
    Tdb_hand = ops.empty_bands(R, A, L, device)
    for r0 in range(0, R, 32):
        ops.edc_curve_db(band_split(measured[r0:r0 + 32], taps, L), L, out=Tdb_hand[r0:r0 + 32])

    def by_hand():
        yk = band_split(infer_bank(bank, sds, taps), taps, L)
        E = torch.flip(torch.cumsum(torch.flip(yk * yk, dims=[-1]), dim=-1), dims=[-1])
        db = torch.clamp(10.0 * torch.log10(E.abs() + EPS), min=-200.0)
        err = (db - Tdb_hand).abs().mean(dim=-1)
        return err, torch.linalg.vector_norm(err, dim=0) / R ** 0.5

    by_hand()
    hand = [wall_ms(by_hand) for _ in range(args.repeats)]
    err_hand = hand[-1][1][0].clone()
    hand = [h[0] for h in hand]
    del Tdb_hand
    torch.cuda.empty_cache()

    # ---- the bank's call
    first_ms, (err, rmse) = wall_ms(lambda: edc_error_bank(bank, sds, taps, measured))
    steady = [wall_ms(lambda: edc_error_bank(bank, sds, taps, measured))[0] for _ in range(args.repeats + 2)][2:]
    parity = float((err - err_hand).abs().max())

    # ---- the launch alone
    Dk = sds.direct_band_render(taps, taps, L)
    Tdb = sds.edc_error_target(measured, taps, L)
    Ck = bank.analysis_group_signals(sds.z_values, taps, taps, L)
    W = bank.render_gains(sds.norm_listener_position, R)
    S = W.shape[1]
    out = torch.empty((R, A), dtype=torch.float32, device=device)
    for _ in range(3):
        ops.edc_error(Dk, Tdb, L, W=W, Ck=Ck, out=out)
    kern = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.edc_error(Dk, Tdb, L, W=W, Ck=Ck, out=out)
        e1.record()
        e1.synchronize()
        kern.append(e0.elapsed_time(e1))
    k_ms = statistics.median(kern)
    nbytes = (2 * R * A * L + A * S * L) * 4
    gbs = nbytes / (k_ms * 1e-3) / 1e9
    res = {'what': 'EDC matching error of a band bank over the receiver grid, ms', 'bands': len(centres),
           'N': bench.G * bench.NPER, 'K': bench.K, 'receivers': R, 'taps': TAPS, 'analysis_bands': A, 'signals': S,
           'samples': L, 'repeats': args.repeats, 'device': torch.cuda.get_device_name(0),
           'constant_bytes_each': R * A * int(Dk.stride(1)) * 4,
           'by_hand': stats(hand), 'bank_first_ms': round(first_ms, 3), 'bank': stats(steady),
           'by_hand_over_bank': round(statistics.median(hand) / statistics.median(steady), 2),
           'bank_vs_by_hand_max_abs_dB': float(f"{parity:.3e}"),
           'rmse_dB': [round(float(v), 4) for v in rmse.cpu()],
           'kernel': dict(stats(kern), compulsory_bytes=nbytes, TBps=round(gbs / 1e3, 3),
                          fraction_of_8TBps=round(gbs / HBM_PEAK_GBS, 4), fma=R * A * S * L)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
