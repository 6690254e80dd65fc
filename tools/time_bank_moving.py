"""Time of a moving listener's render from a band bank (subband.render_moving_listener_bank, csrc/moving.hip) against the
path a user had before it, at the headline shape: 7 octave bands, N = 16 = 4 groups x 4 lines, nfft = 131 072 (K = 65 537),
838 synthetic receivers per band (rooms as in bench.py), 129-tap FIRs (Lr = 131 200), a path of 60 s at 100 ms updates
(P = 600 positions, h = 3200, Fd = 1600 at 32 kHz: n = 2^18, 131 073 bins), a noise stimulus of 5 s (repeated).

One process, the same bank, dataset, taps, path and stimulus for everything; medians of --repeats with the min - max range:
  by_hand          infer_bank(rows=path) -> a Python loop over the positions: the running average of the rows,
                   ``full_convolve`` of the interval's stimulus block with it (three transforms of n points), torch slicing for
                   the cut, the cross-fade and the tail;
  bank_first       render_moving_listener_bank, first call: builds the dataset constant Dh;
  bank             render_moving_listener_bank, steady state;
  launches         the two launches alone (device events around ``hip_ops.moving_compose`` and ``hip_ops.moving_ola``, summed
                   over the chunks of 32 segments), with their compulsory bytes -- compose: P F 8 x 3 (a row of Dh, the block's
                   spectrum, Z) + chunks x S F 8; ola: the segments' covered samples once + the covered span of out read and
                   written per chunk -- the achieved TB/s and their share of the 8 TB/s HBM peak.
Prints ONE JSON line (kept as profiles/r14_bank_moving.json).

    python tools/time_bank_moving.py [--receivers 838] [--repeats 5] [--bands 7] [--seconds 60]
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
UPDATE_MS, ALPHA, FADE_MS, CHUNK = 100.0, 0.5, 50.0, 32
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
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--bands', type=int, default=len(bench.BAND_CENTRES))
    ap.add_argument('--seconds', type=float, default=60.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bank_moving.py measures on the GPU: no device here")
    if args.repeats < 3:
        raise SystemExit("at least 3 repeats")
    from scipy.signal import firwin
    from diffgfdn_amd import hip_ops as ops
    from diffgfdn_amd.bandbank import BandBank, BandStackedDataset
    from diffgfdn_amd.subband import full_convolve, infer_bank, render_moving_listener_bank
    device = torch.device('cuda', 0)
    centres = list(bench.BAND_CENTRES[:args.bands])
    R = args.receivers
    bands = [build_band(device, q, f, R, False) for q, f in enumerate(centres)]
    bank = BandBank([b[0] for b in bands])
    sds = BandStackedDataset([b[1] for b in bands])
    nyq = bench.FS / 2
    taps = torch.tensor(np.stack([firwin(TAPS, [f / np.sqrt(2), min(f * np.sqrt(2), 0.999 * nyq)], pass_zero=False,
                                         fs=bench.FS) for f in centres]), dtype=torch.float32, device=device)
    fs = float(bench.FS)
    h, Fd = int(UPDATE_MS * 1e-3 * fs), int(FADE_MS * 1e-3 * fs)
    P = int(round(args.seconds * 1e3 / UPDATE_MS))
    Lr = 2 * (bench.K - 1) + TAPS - 1
    lfull, total = h + Lr - 1, P * h
    n = 1 << (lfull - 1).bit_length()
    F = n // 2 + 1
    rng = np.random.RandomState(14)
    path = torch.tensor(rng.randint(0, R, P), device=device)
    stim = torch.tensor(rng.randn(int(5 * fs)), dtype=torch.float32, device=device)
    x = stim.repeat(-(-total // stim.numel()))[:total].contiguous()

    # ---- the path by hand
    n_in = torch.linspace(-1.0, 1.0, Fd, device=device)
    fade_in, fade_out = 0.5 * (1.0 + n_in), 0.5 * (1.0 - n_in)

    def by_hand():
        y = infer_bank(bank, sds, taps, rows=path)
        out = torch.zeros((total,), dtype=torch.float32, device=device)
        f = tail = None
        for k in range(P):
            f = y[k] if f is None else ALPHA * y[k] + (1.0 - ALPHA) * f
            s = full_convolve(f.view(1, -1), x[k * h:(k + 1) * h])[0, :min(lfull, total - k * h)]
            a = k * h
            if k:
                out[a:a + Fd] += tail * fade_out + s[:Fd] * fade_in
                out[a + Fd:a + s.numel()] += s[Fd:]
            else:
                out[a:a + s.numel()] += s
            tail = s[-Fd:]
        return out

    by_hand()
    hand = [wall_ms(by_hand) for _ in range(args.repeats)]
    out_hand = hand[-1][1].clone()
    hand = [t[0] for t in hand]
    torch.cuda.empty_cache()

    # ---- the bank's call
    def call():
        return render_moving_listener_bank(bank, sds, taps, path, x, UPDATE_MS, ALPHA, FADE_MS, chunk=CHUNK)
    first_ms, out = wall_ms(call)
    steady = [wall_ms(call)[0] for _ in range(args.repeats + 2)][2:]
    parity = float((out - out_hand).abs().max() / out_hand.abs().max())

    # ---- the two launches alone, chunk by chunk as the call makes them
    Dh = sds.direct_render_spectrum(taps, n)
    W = bank.render_gains(sds.norm_listener_position, R, path)
    Ch = ops.rfft_pow2(bank.filtered_group_signals(sds.z_values, taps), n)
    S = W.shape[1]
    blocks = x.view(P, h)
    ema = torch.empty((F,), dtype=torch.complex64, device=device)
    tails = [torch.empty((Fd,), dtype=torch.float32, device=device) for _ in range(2)]
    res_out = torch.zeros((total,), dtype=torch.float32, device=device)
    comp, ola = [], []
    for rep in range(args.repeats + 1):
        res_out.zero_()
        ev = []
        for i, k0 in enumerate(range(0, P, CHUNK)):
            k1 = min(k0 + CHUNK, P)
            Xh = ops.rfft_pow2(blocks[k0:k1], n)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            Z = ops.moving_compose(Dh, Xh, ema, ALPHA, k0 == 0, W=W[k0:k1], Ch=Ch, rows=path[k0:k1], rows_checked=True)
            e[1].record()
            s = ops.irfft_pow2_fwd(Z, n)
            e[2].record()
            ops.moving_ola(s, k0, P, h, Lr, Fd, res_out, tails[i & 1] if k0 else None, tails[1 - (i & 1)])
            e[3].record()
            ev.append(e)
        torch.cuda.synchronize()
        if rep:                                   # (the first pass warms up)
            comp.append(sum(e[0].elapsed_time(e[1]) for e in ev))
            ola.append(sum(e[2].elapsed_time(e[3]) for e in ev))
    same = bool(torch.equal(res_out, out))          # (the timed launches are the call's)
    chunks = -(-P // CHUNK)
    comp_bytes = P * F * 8 * 3 + chunks * S * F * 8
    seg_samples = sum(min(lfull, total - k * h) for k in range(P))
    span = sum(min(total, (min(k0 + CHUNK, P) - 1) * h + lfull) - k0 * h for k0 in range(0, P, CHUNK))
    ola_bytes = seg_samples * 4 + span * 8

    def launch(ms, nbytes):
        gbs = nbytes / (statistics.median(ms) * 1e-3) / 1e9
        return dict(stats(ms), compulsory_bytes=nbytes, TBps=round(gbs / 1e3, 3), fraction_of_8TBps=round(gbs / HBM_PEAK_GBS, 4))
    res = {'what': 'a moving listener rendered from a band bank, ms', 'bands': len(centres), 'N': bench.G * bench.NPER,
           'K': bench.K, 'receivers': R, 'taps': TAPS, 'signals': S, 'positions': P, 'h': h, 'Fd': Fd, 'Lr': Lr, 'n': n,
           'chunk': CHUNK, 'repeats': args.repeats, 'device': torch.cuda.get_device_name(0), 'Dh_bytes': R * F * 8,
           'by_hand': stats(hand), 'bank_first_ms': round(first_ms, 3), 'bank': stats(steady),
           'by_hand_over_bank': round(statistics.median(hand) / statistics.median(steady), 2),
           'bank_below_by_hand': max(steady) < min(hand), 'bank_vs_by_hand_rel_err': float(f"{parity:.3e}"),
           'launches_equal_call': same, 'compose': launch(comp, comp_bytes), 'ola': launch(ola, ola_bytes)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
