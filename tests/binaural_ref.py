"""Plain float64 numpy restatement of the reference's binaural render of a moving, head-turning listener
(sound_examples.py:356-535 ``binaural_dynamic_rendering``: get_binaural_rir :425-472, binaural_filter_overlap_add :474-535),
pinned to the reference's own output by ``tests/test_binaural_golden.py`` and the yardstick of ``tests/test_gpu_binaural.py``.
The same stock numpy / scipy transforms and convolution as the reference.

    nb = 2^ceil(log2 L),  A_k = rfft(a[path[k]], nb),  Hh = rfft(hrir_sh, nb)
    h = int(update_ms 1e-3 fs),  Fd = int(fade_len_ms 1e-3 fs) (default: h),  total = P h
    x = the stimulus as float32, repeated or cut to total;  x_k = x[k h : (k + 1) h]
    Rw_0 = R_0,  Rw_k = alpha R_k + (1 - alpha) R_{k-1};  Aw_0 = A_0,  Aw_k = alpha A_k + (1 - alpha) A_{k-1}   (no recursion)
    B_k[e][f] = sum_n conj(Hh[n][e][f]) sum_m Rw_k[n][m] Aw_k[m][f];  b_k[e] = irfft(B_k[e], nb)
    s_k[e] = fftconvolve(x_k, b_k[e], 'full')[: min(h + nb - 1, total - k h)]
    out[k h + i][e] += s_k[e][i];  for k >= 1 and i < Fd instead  t_{k-1}[e][i] fade_out[i] + s_k[e][i] fade_in[i]
    fade_in = sqrt(0.5 (1 + linspace(-1, 1, Fd))),  fade_out = sqrt(0.5 (1 - linspace(-1, 1, Fd)))
    t_{k-1}[e] = the LAST Fd samples of the cut s_{k-1}[e]
"""
import numpy as np
from scipy.signal import fftconvolve

from tests.moving_listener_ref import extended_stimulus, ms_to_samps


def transform_length(L: int) -> int:
    return 2 ** int(np.ceil(np.log2(L)))


def fade_windows(Fd: int):
    n = np.linspace(-1.0, 1.0, Fd)
    return np.sqrt(0.5 * (1.0 + n)), np.sqrt(0.5 * (1.0 - n))       # (fade_in, fade_out), :118-127 with uncorr_fade


def brtfs(A, rot, Hh, alpha: float) -> np.ndarray:
    """B (P, 2, Kb) complex128 from the spectra A (P, Ls, Kb) of the path's ambisonic RIRs, the rotation matrices rot
    (P, Ls, Ls) and the HRTFs Hh (Ls, 2, Kb)"""
    A, rot, Hh = np.asarray(A, dtype=np.complex128), np.asarray(rot, dtype=np.float64), np.asarray(Hh, dtype=np.complex128)
    out = np.empty((A.shape[0], 2, A.shape[2]), dtype=np.complex128)
    for k in range(A.shape[0]):
        Rw = rot[k] if k == 0 else alpha * rot[k] + (1.0 - alpha) * rot[k - 1]
        Aw = A[k] if k == 0 else alpha * A[k] + (1.0 - alpha) * A[k - 1]
        rotated = Aw.T @ Rw.T                                       # (Kb, Ls), :463
        out[k] = np.einsum('nrf,fn->fr', np.conj(Hh), rotated).T    # :466
    return out


def overlap_add(segs, h: int, Fd: int) -> np.ndarray:
    """float64 (P h, 2) from the cut two-ear segments segs[k] (len_k, 2): the reference's own loop (:499-533)"""
    if not 1 <= Fd <= h:
        raise ValueError("1 <= Fd <= h")
    total = len(segs) * h
    fade_in, fade_out = fade_windows(Fd)
    out = np.zeros((total, 2))
    prev_tail = np.zeros((Fd, 2))
    for k, s in enumerate(segs):
        a = k * h
        if k > 0:
            n = min(Fd, s.shape[0])
            out[a:a + n] += prev_tail[:n] * fade_out[:n, None] + s[:n] * fade_in[:n, None]
            out[a + n:a + s.shape[0]] += s[n:]
        else:
            out[a:a + s.shape[0]] += s
        prev_tail[:Fd] = s[-Fd:]                                    # (len_k >= h >= Fd)
    return out


def segments(brirs, x, h: int):
    """the cut two-ear segments of the BRIRs (P, nb, 2)"""
    P = brirs.shape[0]
    total = P * h
    out = []
    for k in range(P):
        xk = x[k * h:(k + 1) * h]
        s = np.stack([fftconvolve(xk, brirs[k, :, e], mode='full') for e in range(2)], axis=1)
        out.append(s[:min(s.shape[0], total - k * h)])
    return out


def ref_binaural(ambi_rirs, hrir_sh, path, rotations, stimulus, fs: float, update_ms: float = 100.0, alpha: float = 0.5,
                 fade_len_ms=None) -> np.ndarray:
    """float64 (P h, 2).  ambi_rirs (R, Ls, L), hrir_sh (Ls, 2, Mh <= nb), path: P rows (None: all in order), rotations
    (P, Ls, Ls)"""
    a = np.asarray(ambi_rirs, dtype=np.float64)
    path = list(range(a.shape[0])) if path is None else [int(p) for p in path]
    h = ms_to_samps(update_ms, fs)
    Fd = h if fade_len_ms is None else ms_to_samps(fade_len_ms, fs)
    if not path or h < 1:
        raise ValueError("P >= 1 and h >= 1")
    nb = transform_length(a.shape[2])
    hr = np.asarray(hrir_sh, dtype=np.float64)
    if hr.shape[2] > nb:
        raise ValueError("the HRIRs are longer than the transform")
    if np.shape(rotations) != (len(path), a.shape[1], a.shape[1]):
        raise ValueError("rotations (P, Ls, Ls)")
    A = np.fft.rfft(a[path], n=nb, axis=-1)
    Hh = np.fft.rfft(hr, n=nb, axis=-1)
    brirs = np.fft.irfft(brtfs(A, rotations, Hh, alpha), n=nb, axis=-1).transpose(0, 2, 1)     # (P, nb, 2)
    x = extended_stimulus(stimulus, len(path) * h)
    return overlap_add(segments(brirs, x, h), h, Fd)
