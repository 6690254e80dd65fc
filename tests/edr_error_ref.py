"""The reference's EDR matching error (plot.py:782-822 ``get_edr_error``) restated on the oracle's STFT and EDR
(``oracle.gfdn_oracle.stft_onesided`` / ``edr_from_stft`` / ``db``: losses.py:501-575, utils.py:16-40), for the tests of
``subband.edr_error_bank``.

  1. L = min(Tx, Ty); both sides cut to L                                              (plot.py:848-852)
  2. STFT: zero-padded to whole hops, periodic Hann of ``win``, hop = win / 2, nfft = win, center=False, one-sided
  3. EDR[f][m] = dB(sum_{tau >= m} |S[f][tau]|^2), dB(v) = max(10 log10(|v| + eps_f32), -200)
  4. error_db[r] = mean_{f, m} |EDR_x - EDR_y|, rmse = ||error_db||_2 / sqrt(R)           (plot.py:818-821)

The reference keeps the EDR in a float32 buffer (losses.py:566-574): the tail sums are rounded to float32, the dB stage and
the mean of step 4 run in float32.  ``reference_rounding=True`` restates exactly that (``edr_from_stft``);  the default takes
tail sums, dB and mean in float64 -- the yardstick of the GPU tests.  ``tests/test_edr_error_golden.py`` pins the first to
the reference's own output and bounds the distance between the two."""
import numpy as np
import torch

from oracle.gfdn_oracle import db, edr_from_stft, stft_onesided


def edr_db(x, win: int, reference_rounding: bool = False) -> np.ndarray:
    """(rows, F, T): EDR in dB of the rows of ``x`` (rows, L), transformed in float64 (the window is the float32 periodic
    Hann of torch.hann_window, as in the reference).  float32 with ``reference_rounding``, else float64."""
    S = stft_onesided(torch.as_tensor(np.asarray(x, dtype=np.float64)), win, win // 2)
    if reference_rounding:
        return edr_from_stft(S).numpy()
    E = torch.flip(torch.cumsum(torch.flip(torch.abs(S) ** 2, dims=[-1]), dim=-1), dims=[-1])
    return db(E, is_squared=True).numpy()


def ref_edr_error(estimated, measured, win: int = 4096, reference_rounding: bool = False):
    """(error_db (R,), rmse) of estimated (R, Ty) against measured (R, Tx): plot.py:848-852 and :818-821"""
    estimated, measured = np.asarray(estimated), np.asarray(measured)
    L = min(estimated.shape[-1], measured.shape[-1])
    original_edr = edr_db(measured[..., :L], win, reference_rounding)
    est_edr = edr_db(estimated[..., :L], win, reference_rounding)
    error_db = np.abs(original_edr - est_edr).mean(axis=(1, 2))
    return error_db, np.linalg.norm(error_db) / np.sqrt(error_db.shape[0])
