"""Time of the spatial render of the directional bands (subband.infer_directional_bands, csrc/dirrender.hip) against the
band-by-band render it replaces and against the stock-operator formulations of its mix, at the config-4 shape of bench.py:
7 octave bands, G = 3 groups x 9 lines (2nd-order ambisonics), J = 12 directions, nfft = 131 072 (K = 65 537), 838
receivers, 129-tap reconstructing FIRs, length = 64 000 samples (the reference's edc_len_ms = 2000 at 32 kHz).

One process, the same nets, positions, taps and analysis matrix for everything:
  by_hand     band by band, batches of 32 receivers: get_response -> cut -> sh_to_directional -> same-mode convolution ->
              accumulate (once: it is the slow path);
  infer       subband.infer_directional_bands, directional and ambisonic output (median of --repeats, host clock);
  launch      the ``hip_ops.dir_render`` launch alone (device events), both modes, with its compulsory bytes (the output
              plus one read of C and W) , the achieved GB/s and their share of the 8 TB/s HBM peak;
  two_stage   ``subband.directional_mix_torch`` on the same W, C, A: Ls skinny products, then the J x Ls contraction;
  folded      A folded into the weights, one (R J) x (S Ls) x L product.
Prints ONE JSON line.

    python tools/time_directional_render.py [--receivers 838] [--repeats 9] [--bands 7]
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

import bench  # noqa: E402  (the config-4 workload's constants)

TAPS, LENGTH, BATCH = 129, 64000, 32
HBM_PEAK_GBS = 8000.0


def wall_ms(fn):
    """host clock around work that ends in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn, repeats):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def build_nets(device, nb, Gd=3, order=2, J=12):
    from diffgfdn_amd.config import CouplingMatrixType, DiffGFDNConfig, FeedbackLoopConfig, OutputFilterConfig
    from diffgfdn_amd.model import DiffDirectionalFDNVarReceiverPos
    Ls = (order + 1) ** 2
    A = np.random.RandomState(7).randn(J, Ls).astype(np.float32)          # (one analysis matrix for all bands)
    nets = []
    for q in range(nb):
        torch.manual_seed(500 + q)
        delays = DiffGFDNConfig(num_groups=Gd, num_delay_lines=Gd * Ls, sample_rate=bench.FS,
                                seed=23463 + q).delay_length_samps
        fl = FeedbackLoopConfig(coupling_matrix_type=CouplingMatrixType.SCALAR, use_zero_coupling=True)
        of = OutputFilterConfig(use_svfs=False, num_hidden_layers=5, num_neurons_per_layer=16, num_fourier_features=20)
        nets.append(DiffDirectionalFDNVarReceiverPos(bench.FS, Gd, delays, device, fl, of, ambi_order=order,
                                                     common_decay_times=np.linspace(0.5, 1.4, Gd)[None, :],
                                                     use_colorless_loss=True, analysis_matrix=A).to(device))
    return nets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--receivers', type=int, default=838)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--bands', type=int, default=len(bench.BAND_CENTRES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_directional_render.py measures on the GPU: no device here")
    if args.repeats < 5:
        raise SystemExit("at least 5 repeats")
    from scipy.signal import firwin
    from diffgfdn_amd import hip_ops as ops
    from diffgfdn_amd.subband import (directional_band_signals, directional_mix_torch, full_convolve,
                                      infer_directional_bands)
    from diffgfdn_amd.trainer import get_response
    device = torch.device('cuda', 0)
    centres = list(bench.BAND_CENTRES[:args.bands])
    R, K = args.receivers, bench.K
    nets = build_nets(device, len(centres))
    G, Ls = nets[0].num_groups, nets[0].num_delay_lines_per_group
    A = nets[0].sh_output_scalars.analysis_matrix
    J = A.shape[0]
    rng = np.random.RandomState(11)
    z = torch.exp(1j * np.pi * torch.arange(K, dtype=torch.float64) / (K - 1)).to(device)
    pos = torch.tensor(rng.uniform(0, 1, (R, 3)), device=device)
    lpos = torch.tensor(rng.uniform(0, 10, (R, 3)), device=device)
    nyq = bench.FS / 2
    taps = torch.tensor(np.stack([firwin(TAPS, [f / np.sqrt(2), min(f * np.sqrt(2), 0.999 * nyq)], pass_zero=False,
                                         fs=bench.FS) for f in centres]), dtype=torch.float32, device=device)
    L = min(LENGTH, 2 * (K - 1))
    sh = (TAPS - 1) // 2

    def by_hand(receivers):
        out = torch.zeros((receivers, J, L), dtype=torch.float32, device=device)
        for q, net in enumerate(nets):
            for r0 in range(0, receivers, BATCH):
                r1 = min(r0 + BATCH, receivers)
                x = {'z_values': z, 'listener_position': lpos[r0:r1], 'norm_listener_position': pos[r0:r1]}
                h = get_response(x, net)[-1][..., :L].contiguous()
                hc = torch.view_as_complex(h.view(r1 - r0, Ls, L // 2, 2))
                d = torch.view_as_real(ops.sh_to_directional(A, hc)).reshape((r1 - r0) * J, L)
                out[r0:r1] += full_convolve(d, taps[q])[:, sh:sh + L].reshape(r1 - r0, J, L)
        return out

    by_hand(BATCH)                                                     # warm-up of every kernel of the slow path
    hand_ms, y_hand = wall_ms(lambda: by_hand(R))
    out_dir = torch.empty((R, J, L), dtype=torch.float32, device=device)
    infer_directional_bands(nets, z, pos, taps, L, out=out_dir)
    parity = float((out_dir - y_hand).abs().max()) / float(y_hand.abs().max())
    del y_hand
    infer_dir = [wall_ms(lambda: infer_directional_bands(nets, z, pos, taps, L, out=out_dir))[0]
                 for _ in range(args.repeats + 2)][2:]
    out_ambi = torch.empty((R, Ls, L), dtype=torch.float32, device=device)
    infer_ambi = [wall_ms(lambda: infer_directional_bands(nets, z, pos, taps, L, directional=False, out=out_ambi))[0]
                  for _ in range(args.repeats + 2)][2:]

    # the launch alone, and the stock-operator formulations on the same W, C, A
    with torch.no_grad():
        C = directional_band_signals(nets, z, taps, L)
        W = torch.stack([net.sh_output_scalars({'norm_listener_position': pos}, normalise_weights=True) for net in nets],
                        dim=1).reshape(R, -1, Ls).contiguous()
    S = W.shape[1]
    launch_dir = event_ms(lambda: ops.dir_render(W, C, Ls, a=A, out=out_dir), args.repeats)
    launch_ambi = event_ms(lambda: ops.dir_render(W, C, Ls, out=out_ambi), args.repeats)
    ref = out_dir.clone()
    two_stage = event_ms(lambda: directional_mix_torch(W, C, Ls, A, out_dir), args.repeats)
    two_stage_err = float((out_dir - ref).abs().max()) / float(ref.abs().max())
    Cc = C.contiguous()

    def folded():
        WA = torch.einsum('jl,rsl->rjsl', A, W).reshape(R * J, S * Ls)
        torch.matmul(WA, Cc, out=out_dir.view(R * J, L))
    folded_ms = event_ms(folded, args.repeats)
    folded_err = float((out_dir - ref).abs().max()) / float(ref.abs().max())

    def rate(ms, rows):
        nbytes = (R * rows * L + S * Ls * L + R * S * Ls) * 4
        gbs = nbytes / (ms * 1e-3) / 1e9
        return {'compulsory_bytes': nbytes, 'GBps': round(gbs, 1), 'fraction_of_8TBps': round(gbs / HBM_PEAK_GBS, 4)}
    flop_dir, flop_ambi = 2 * R * L * (S * Ls + J * Ls), 2 * R * L * S * Ls
    launch_dir.update(rate(launch_dir['median_ms'], J), flop=flop_dir,
                      TFLOPs=round(flop_dir / (launch_dir['median_ms'] * 1e-3) / 1e12, 2))
    launch_ambi.update(rate(launch_ambi['median_ms'], Ls), flop=flop_ambi,
                       TFLOPs=round(flop_ambi / (launch_ambi['median_ms'] * 1e-3) / 1e12, 2))
    best_torch = min(two_stage['median_ms'], folded_ms['median_ms'])

    def med(v):
        return {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4)}
    out = {'what': 'spatial render of the directional bands, ms', 'bands': len(centres), 'groups': G, 'channels': Ls,
           'directions': J, 'K': K, 'receivers': R, 'taps': TAPS, 'signals': S * Ls, 'samples': L, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0),
           'by_hand_ms': round(hand_ms, 3), 'by_hand_batch': BATCH,
           'infer_directional': med(infer_dir), 'infer_ambisonic': med(infer_ambi),
           'by_hand_over_infer_directional': round(hand_ms / statistics.median(infer_dir), 2),
           'infer_vs_by_hand_rel_err': float(f"{parity:.3e}"),
           'launch_directional': launch_dir, 'launch_ambisonic': launch_ambi,
           'torch_two_stage': dict(two_stage, rel_err=float(f"{two_stage_err:.3e}")),
           'torch_folded': dict(folded_ms, rel_err=float(f"{folded_err:.3e}"), flop=2 * R * J * S * Ls * L),
           'faster_torch_over_launch_directional': round(best_torch / launch_dir['median_ms'], 2)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
