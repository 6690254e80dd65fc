#!/usr/bin/env python
"""Golden vector of the spatial render of the directional bands (f19_directional_render.npz): the reference's own chain of
``infer_all_octave_bands_directional_fdn`` (inference.py:676-881) on three small bands.

Per band: the reference's DiffDirectionalFDNVarReceiverPos at the ``f6_directional.npz`` size (fs = 8 kHz, nfft = 1024,
G = 2, order 1, J = 5, three receivers) -- band 0 with that fixture's parameters, bands 1 and 2 with the perturbed copies
that ``_directional_bands`` of tests/test_gpu_parity.py builds (same generator seeds) -- through ``get_response``
(utils.py:149-179), the cut to ``length`` = 700 of 1024 samples, ``InferDiffDirectionalFDN.convert_ambi_rir_to_directional_rir``
(:387-400) when the directional RIRs are asked for, ``scipy.signal.fftconvolve(rir, taps[None, :], mode='same')`` (:807-810)
and the float32 sum over the bands per receiver (:848-857).  Two sets of reconstructing FIRs: M = 129 (odd) and M = 64
(even) taps.  The classes are imported unmodified; the analysis matrix is the fixture's (spaudiopy is absent), patched in as
``gen_golden.gen_f6_directional`` does.  Run from the repository root where the reference sources are present:

    python tests/golden/gen_f19_directional_render.py
"""
import os
import sys
import types

import numpy as np
import torch
from scipy.signal import fftconvolve

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.install()
from diff_gfdn.config.config import CouplingMatrixType, FeedbackLoopConfig, OutputFilterConfig  # noqa: E402
from diff_gfdn.inference import InferDiffDirectionalFDN  # noqa: E402
from diff_gfdn.model import DiffDirectionalFDNVarReceiverPos  # noqa: E402
from diff_gfdn.utils import get_response  # noqa: E402
import spatial_sampling.model as ss_model  # noqa: E402

NB, LENGTH, TAPS = 3, 700, (129, 64)
PERTURBED = ("input_gains", "output_gains", "feedback_loop.M")


def band_state(fx, q):
    """the state dict of band q as ``_directional_bands`` (tests/test_gpu_parity.py) forms it"""
    sd = {k[3:]: torch.tensor(v) for k, v in fx.items() if k.startswith("sd_")}
    if q:
        g = torch.Generator().manual_seed(77 + q)
        sd = {k: (v + 0.05 * torch.randn(v.shape, generator=g).to(v.dtype) if v.is_floating_point() and k in PERTURBED
                  else v) for k, v in sd.items()}
    return sd


def main():
    fx = dict(np.load(os.path.join(HERE, "f6_directional.npz")))
    fs, G, order = float(fx["fs"]), int(fx["G"]), int(fx["order"])
    analysis = fx["analysis_matrix"].astype(np.float32)
    J = analysis.shape[0]

    def fake_init(self, beamformer_type, desired_directions):
        self.modal_weights = np.ones(self.ambi_order + 1)
        self.analysis_matrix = torch.tensor(analysis, dtype=torch.float32)

    ss_model.Directional_Beamforming_Weights.initialise_beamformer = fake_init
    batch = {k[6:]: torch.tensor(v) for k, v in fx.items() if k.startswith("batch_")}
    rng = np.random.RandomState(19)
    taps = {M: (rng.randn(NB, M) * np.hanning(M + 2)[1:-1]).astype(np.float32) for M in TAPS}
    fl = FeedbackLoopConfig(coupling_matrix_type=CouplingMatrixType.SCALAR, use_zero_coupling=True)
    of = OutputFilterConfig(use_svfs=False, num_hidden_layers=1, num_neurons_per_layer=8, num_fourier_features=3,
                            use_skip_connections=False)
    save = dict(length=np.int64(LENGTH), num_bands=np.int64(NB), **{f"taps_{M}": t for M, t in taps.items()})
    total = {(M, d): 0 for M in TAPS for d in (True, False)}
    for q in range(NB):
        torch.manual_seed(900 + q)
        net = DiffDirectionalFDNVarReceiverPos(fs, G, fx["delays"].tolist(), 'cpu', fl, of, ambi_order=order,
                                               desired_directions=np.zeros((2, J)),
                                               common_decay_times=(fx["T60"] * (1.0 + 0.15 * q))[None, :],
                                               use_colorless_loss=True)
        sd = band_state(fx, q)
        net.load_state_dict(sd, strict=True)
        net.eval()
        for k in PERTURBED:
            save[f"b{q}_{k}"] = sd[k].numpy().copy()
        with torch.no_grad():
            _, _, ambi = get_response(batch, net)                                      # (R, Ls, nfft)
            owner = types.SimpleNamespace(model=net)
            rirs = {True: InferDiffDirectionalFDN.convert_ambi_rir_to_directional_rir(owner, ambi)[..., :LENGTH],
                    False: ambi[..., :LENGTH]}
        assert ambi.shape[-1] == int(fx["nfft"]) > LENGTH
        for (M, d) in total:
            for r in range(ambi.shape[0]):
                cur = rirs[d][r].detach().cpu().numpy()
                filt = fftconvolve(cur, taps[M][q][None, :], mode='same').astype(np.float32)
                if isinstance(total[(M, d)], int):
                    total[(M, d)] = np.zeros((ambi.shape[0],) + filt.shape, dtype=np.float32)
                total[(M, d)][r] += filt
    for (M, d), v in total.items():
        save[f"{'dir' if d else 'ambi'}_{M}"] = v
        print(f"M = {M}, {'directional' if d else 'ambisonic'}: {v.shape}, |out| <= {np.abs(v).max():.4f}")
    np.savez_compressed(os.path.join(HERE, "f19_directional_render.npz"), **save)


if __name__ == "__main__":
    main()
