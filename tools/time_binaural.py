"""Time of the binaural render of a moving, head-turning listener from the directional bands
(subband.render_binaural_moving_listener_bands, csrc/binaural.hip) against the route a user had before it, at the config-4
shape: 838 receivers, 7 directional bands (3 groups each: S = 21 band signals per channel), order 2 (Ls = 9), length 64 000
(nb = 65 536, Kb = 32 769, n2 = 131 072), a path of P = 600 positions at 100 ms and 48 kHz (h = Fd = 4800), a synthetic
256-tap SH HRIR set, yaw-only rotations built here (degree l: a plane rotation by m yaw of every (-m, +m) pair), a noise
stimulus of 5 s (repeated).

One process, the same nets, HRIRs, path, rotations and stimulus for everything:
  by_hand     infer_directional_bands(directional=False, rows=path) -> torch rfft of the P x Ls RIRs at nb -> a Python loop
              per position: interpolation, rotation, HRTF product, irfft, two ``full_convolve`` calls, torch slicing for the
              cut, the cross-fade and the tail;
  call        render_binaural_moving_listener_bands, steady state (medians of --repeats with the min - max range);
  launches    the two launches alone (device events around ``hip_ops.binaural_compose`` and ``hip_ops.binaural_ola``, summed
              over the chunks of 32 segments), with the bytes each moves -- compose: per chunk the S Ls spectra of C^ once
              per segment tile of 16 and the 2 Ls HRTF rows once per tile, plus P x 2 x Kb x 8 written; ola: the segments'
              covered samples of both ears once + the covered span of out read and written per chunk -- the achieved TB/s
              and their share of the 8 TB/s HBM peak.
Prints ONE JSON line (kept as profiles/r16_binaural.json).

    python tools/time_binaural.py [--receivers 838] [--repeats 5] [--bands 7] [--positions 600]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402  (the config-4 workload's constants)
from time_directional_render import build_nets, wall_ms  # noqa: E402

TAPS, LENGTH, MH = 129, 64000, 256
UPDATE_MS, ALPHA, CHUNK, TILE = 100.0, 0.5, 32, 16
HBM_PEAK_GBS = 8000.0


def stats(ms):
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def yaw_rotations(yaw, order):
    """(P, Ls, Ls) real SH rotation matrices of a rotation about z (ACN order): per degree l and m >= 1 the pair (-m, +m)
    turns by m yaw"""
    Ls = (order + 1) ** 2
    out = np.zeros((len(yaw), Ls, Ls), dtype=np.float32)
    for l in range(order + 1):
        c0 = l * l + l
        out[:, c0, c0] = 1.0
        for m in range(1, l + 1):
            c, s = np.cos(m * yaw), np.sin(m * yaw)
            out[:, c0 + m, c0 + m], out[:, c0 - m, c0 - m] = c, c
            out[:, c0 + m, c0 - m], out[:, c0 - m, c0 + m] = -s, s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--receivers', type=int, default=838)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--bands', type=int, default=len(bench.BAND_CENTRES))
    ap.add_argument('--positions', type=int, default=600)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_binaural.py measures on the GPU: no device here")
    if args.repeats < 3:
        raise SystemExit("at least 3 repeats")
    from scipy.signal import firwin
    from diffgfdn_amd import hip_ops as ops
    from diffgfdn_amd.subband import (_directional_inputs, full_convolve, infer_directional_bands,
                                      render_binaural_moving_listener_bands)
    device = torch.device('cuda', 0)
    centres = list(bench.BAND_CENTRES[:args.bands])
    R, K, P = args.receivers, bench.K, args.positions
    nets = build_nets(device, len(centres))
    G, Ls = nets[0].num_groups, nets[0].num_delay_lines_per_group
    S = len(nets) * G
    fs = 48000.0                                                       # (the listener's rate; the nets keep bench.FS)
    rng = np.random.RandomState(16)
    z = torch.exp(1j * np.pi * torch.arange(K, dtype=torch.float64) / (K - 1)).to(device)
    pos = torch.tensor(rng.uniform(0, 1, (R, 3)), device=device)
    nyq = bench.FS / 2
    taps = torch.tensor(np.stack([firwin(TAPS, [f / np.sqrt(2), min(f * np.sqrt(2), 0.999 * nyq)], pass_zero=False,
                                         fs=bench.FS) for f in centres]), dtype=torch.float32, device=device)
    L = min(LENGTH, 2 * (K - 1))
    nb = 1 << (L - 1).bit_length()
    Kb = nb // 2 + 1
    h = Fd = int(UPDATE_MS * 1e-3 * fs)
    lfull, total = h + nb - 1, P * h
    n2 = 1 << (lfull - 1).bit_length()
    path = torch.tensor(rng.randint(0, R, P), device=device)
    rot = torch.tensor(yaw_rotations(np.cumsum(rng.uniform(-0.2, 0.2, P)), int(round(Ls ** 0.5)) - 1), device=device)
    hrir = torch.tensor((rng.randn(Ls, 2, MH) * np.exp(-np.arange(MH) / 40.0)).astype(np.float32), device=device)
    stim = torch.tensor(rng.randn(int(5 * fs)), dtype=torch.float32, device=device)
    x = stim.repeat(-(-total // stim.numel()))[:total].contiguous()

    # ---- the route by hand
    n_in = torch.linspace(-1.0, 1.0, Fd, device=device)
    fade_in, fade_out = torch.sqrt(0.5 * (1.0 + n_in))[:, None], torch.sqrt(0.5 * (1.0 - n_in))[:, None]
    Hc = torch.fft.rfft(hrir, n=nb).conj()

    def by_hand():
        a = infer_directional_bands(nets, z, pos, taps, L, directional=False, rows=path)
        out = torch.zeros((total, 2), dtype=torch.float32, device=device)
        Ap = Rp = tail = None
        for k in range(P):
            Ak = torch.fft.rfft(a[k], n=nb)
            Aw = Ak if Ap is None else ALPHA * Ak + (1.0 - ALPHA) * Ap
            Rw = rot[k] if Rp is None else ALPHA * rot[k] + (1.0 - ALPHA) * Rp
            Ap, Rp = Ak, rot[k]
            B = torch.einsum('nef,nf->ef', Hc, Rw.to(Aw.dtype) @ Aw)
            brir = torch.fft.irfft(B, n=nb)
            s = full_convolve(brir, x[k * h:(k + 1) * h])[:, :min(lfull, total - k * h)].T
            a0 = k * h
            if k:
                out[a0:a0 + Fd] += tail * fade_out + s[:Fd] * fade_in
                out[a0 + Fd:a0 + s.shape[0]] += s[Fd:]
            else:
                out[a0:a0 + s.shape[0]] += s
            tail = s[-Fd:]
        return out

    hand = [wall_ms(by_hand) for _ in range(2)]
    out_hand = hand[-1][1]
    hand = [t[0] for t in hand][1:]
    torch.cuda.empty_cache()

    # ---- the call
    def call():
        return render_binaural_moving_listener_bands(nets, z, pos, taps, L, hrir, path, rot, x, UPDATE_MS, ALPHA,
                                                     sample_rate=fs, chunk=CHUNK)
    first_ms, out = wall_ms(call)
    steady = [wall_ms(call)[0] for _ in range(args.repeats + 1)][1:]
    parity = float((out - out_hand).abs().max() / out_hand.abs().max())
    del out_hand

    # ---- the two launches alone, chunk by chunk as the call makes them
    W, C, _, _ = _directional_inputs(nets, z, pos, taps, L, path, 4096, "time_binaural")
    Ch = ops.rfft_pow2(C, nb)
    Hh = ops.rfft_pow2(hrir.reshape(Ls * 2, MH), nb).view(Ls, 2, Kb)
    blocks = x.view(P, h)
    tails = [torch.empty((Fd, 2), dtype=torch.float32, device=device) for _ in range(2)]
    res_out = torch.zeros((total, 2), dtype=torch.float32, device=device)
    comp, ola = [], []
    for rep in range(args.repeats + 1):
        res_out.zero_()
        ev = []
        for i, k0 in enumerate(range(0, P, CHUNK)):
            k1 = min(k0 + CHUNK, P)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            B = ops.binaural_compose(rot, Hh, ALPHA, k0, k1 - k0, W=W, Ch=Ch)
            e[1].record()
            brir = ops.irfft_pow2_fwd(B.reshape(-1, Kb), nb)
            Z = ops.rfft_pow2(brir, n2).view(k1 - k0, 2, -1) * ops.rfft_pow2(blocks[k0:k1], n2).unsqueeze(1)
            s = ops.irfft_pow2_fwd(Z.view(2 * (k1 - k0), -1), n2).view(k1 - k0, 2, n2)
            e[2].record()
            ops.binaural_ola(s, k0, P, h, nb, Fd, res_out, tails[i & 1] if k0 else None, tails[1 - (i & 1)])
            e[3].record()
            ev.append(e)
        torch.cuda.synchronize()
        if rep:                                   # (the first pass warms up)
            comp.append(sum(e[0].elapsed_time(e[1]) for e in ev))
            ola.append(sum(e[2].elapsed_time(e[3]) for e in ev))
    same = bool(torch.equal(res_out, out))          # (the timed launches are the call's)
    tiles = sum(-(-(min(k0 + CHUNK, P) - k0) // TILE) for k0 in range(0, P, CHUNK))
    comp_bytes = tiles * (S * Ls + 2 * Ls) * Kb * 8 + P * 2 * Kb * 8
    seg_samples = sum(min(lfull, total - k * h) for k in range(P))
    span = sum(min(total, (min(k0 + CHUNK, P) - 1) * h + lfull) - k0 * h for k0 in range(0, P, CHUNK))
    ola_bytes = seg_samples * 8 + span * 16

    def launch(ms, nbytes):
        gbs = nbytes / (statistics.median(ms) * 1e-3) / 1e9
        return dict(stats(ms), bytes=nbytes, TBps=round(gbs / 1e3, 3), fraction_of_8TBps=round(gbs / HBM_PEAK_GBS, 4))
    fma = P * Kb * Ls * (2 * S + 4 * Ls + 14)
    res = {'what': 'a moving, head-turning listener rendered binaurally from the directional bands, ms', 'bands': len(centres),
           'groups': G, 'channels': Ls, 'signals_per_channel': S, 'receivers': R, 'taps': TAPS, 'length': L, 'nb': nb,
           'n2': n2, 'positions': P, 'h': h, 'Fd': Fd, 'hrir_taps': MH, 'chunk': CHUNK, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0), 'by_hand': stats(hand), 'call_first_ms': round(first_ms, 3),
           'call': stats(steady), 'by_hand_over_call': round(statistics.median(hand) / statistics.median(steady), 2),
           'call_vs_by_hand_rel_err': float(f"{parity:.3e}"), 'launches_equal_call': same,
           'compose': dict(launch(comp, comp_bytes), lane_fmas=fma,
                           Tfma_per_s=round(fma / (statistics.median(comp) * 1e-3) / 1e12, 2)),
           'ola': launch(ola, ola_bytes)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
