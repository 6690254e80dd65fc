#!/usr/bin/env python
"""Golden vector of the EDR matching error (f17_edr_error.npz): the reference's own ``get_stft_torch`` and
``get_edr_from_stft`` (losses.py:501-575) on a small seeded problem, then plot.py:848-852 (both sides cut to the shorter
length) and :818-821 (mean |difference| over frequency and time per receiver, norm / sqrt(R)) applied literally.

``get_edr_error`` itself is a closure of ``plot_edr_error_in_space`` that needs a room and a plot; the lines it runs on the
RIRs are the ones below.  Run from the repository root where the reference sources are present:

    python tests/golden/gen_f17_edr_error.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.install()
from diff_gfdn.losses import get_edr_from_stft, get_stft_torch  # noqa: E402
from diff_gfdn.utils import db as ref_db  # noqa: E402

R, WIN, HOP, FS = 5, 512, 256, 48000.0
TX, TY = 2301, 2075                 # different lengths, neither a multiple of the hop


def decaying_noise(rng, rows, T, amp, tau):
    return amp * np.exp(-np.arange(T) / tau) * rng.randn(rows, T)


def main():
    rng = np.random.RandomState(17)
    # the measured side reaches the eps floor (-69.2 dB) in its last frames; the estimate is 1.4 times as loud and decays
    # a little more slowly
    measured = decaying_noise(rng, R, TX, 2e-2, 180.0)
    estimated = decaying_noise(rng, R, TY, 2.8e-2, 200.0)

    rir_len_samps = min(measured.shape[-1], estimated.shape[-1])                    # plot.py:848-852
    cur_est_rirs = estimated[..., :rir_len_samps]
    cur_original_rirs = measured[..., :rir_len_samps]
    S_orig, _, _ = get_stft_torch(torch.tensor(cur_original_rirs.copy()), FS, win_size=WIN, hop_size=HOP, nfft=WIN)
    original_edr = get_edr_from_stft(S_orig).cpu().detach().numpy()
    S_est, _, _ = get_stft_torch(torch.tensor(cur_est_rirs.copy()), FS, win_size=WIN, hop_size=HOP, nfft=WIN)
    est_edr = get_edr_from_stft(S_est).cpu().detach().numpy()
    error_db = np.abs(original_edr - est_edr).mean(axis=(1, 2))                     # plot.py:818-821
    error_mse = np.linalg.norm(error_db) / np.sqrt(R)

    # the same lines with the reference's float32 EDR buffer (losses.py:566-574) widened to float64: its own STFT, its own
    # tail sums and its own dB (utils.py:16-40), nothing rounded to float32 -- what a float64 restatement can be held to on
    # any machine (a float32 rounding flips where the float64 value behind it moves in its last bits)
    def edr64(S):
        edr = torch.zeros(S.shape, dtype=torch.float64)
        for m in range(S.shape[-1]):
            edr[..., m] = torch.sum(torch.abs(S[..., m:])**2, axis=-1)
        return ref_db(edr, is_squared=True).numpy()
    error_db_f64 = np.abs(edr64(S_orig) - edr64(S_est)).mean(axis=(1, 2))
    rmse_f64 = np.linalg.norm(error_db_f64) / np.sqrt(R)

    floor = float(original_edr.min())
    on_floor = float((original_edr <= floor + 1e-3).mean())
    print(f"EDR (rows, F, T) = {original_edr.shape}, measured side {original_edr.max():.1f} .. {floor:.2f} dB, "
          f"{100 * on_floor:.0f} % of its cells on the eps floor; error_db {np.round(error_db, 3)}, rmse {error_mse:.4f}")
    assert 0.1 < on_floor < 0.9, "part of the EDR sits on the eps floor, part above"
    np.savez_compressed(os.path.join(HERE, "f17_edr_error.npz"), measured=measured, estimated=estimated,
                        win=np.int64(WIN), original_edr=original_edr, est_edr=est_edr, error_db=error_db,
                        rmse=np.asarray(error_mse), error_db_f64=error_db_f64, rmse_f64=np.asarray(rmse_f64))


if __name__ == "__main__":
    main()
