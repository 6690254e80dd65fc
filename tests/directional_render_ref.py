"""Float64 restatement of the spatial render of the directional bands (subband.infer_directional_bands, csrc/dirrender.hip),
in numpy: the formulas of the reference's ``infer_all_octave_bands_directional_fdn`` (inference.py:676-881) with the
receiver factored out.

    C[q][g][l]    = same_conv(irfft(lines[q][g][l], n = 2 (K - 1))[:length], taps[q])      lines = c_{g,l} Y_q[:, g Ls + l]
    ambi[r][l][t] = sum_{q,g} w[q][r][g][l] C[q][g][l][t]
    dir[r][j][t]  = sum_l A[j][l] ambi[r][l][t]
"""
import numpy as np


def same_conv(x, taps):
    """scipy.signal.fftconvolve(x, taps[None, :], mode='same') along the last axis, written out: the len(x) samples of the
    full convolution from sample (M - 1) // 2 on."""
    x, taps = np.asarray(x, dtype=np.float64), np.asarray(taps, dtype=np.float64)
    L, M = x.shape[-1], taps.shape[-1]
    full = np.zeros(x.shape[:-1] + (L + M - 1,))
    for m in range(M):
        full[..., m:m + L] += taps[m] * x
    s = (M - 1) // 2
    return full[..., s:s + L]


def band_signals(lines, taps, length):
    """C (Q, G, Ls, L): lines (Q, G, Ls, K) complex spectra of the delay lines with their output gains, taps (Q, M)"""
    lines = np.asarray(lines, dtype=np.complex128)
    n = 2 * (lines.shape[-1] - 1)
    L = min(int(length), n)
    h = np.fft.irfft(lines, n=n, axis=-1)[..., :L]
    return np.stack([same_conv(h[q], taps[q]) for q in range(lines.shape[0])])


def mix(W, C, A=None):
    """W (R, S, Ls), C (S, Ls, n) -> ambi (R, Ls, n), or (R, J, n) with A (J, Ls)"""
    ambi = np.einsum('rsl,sln->rln', np.asarray(W, dtype=np.float64), np.asarray(C, dtype=np.float64))
    return ambi if A is None else np.einsum('jl,rln->rjn', np.asarray(A, dtype=np.float64), ambi)


def render(lines, w, taps, length, A=None):
    """lines (Q, G, Ls, K), w (Q, R, G, Ls), taps (Q, M) -> (R, J or Ls, L) float64"""
    C = band_signals(lines, taps, length)
    Q, G, Ls, L = C.shape
    W = np.asarray(w, dtype=np.float64).transpose(1, 0, 2, 3).reshape(-1, Q * G, Ls)
    return mix(W, C.reshape(Q * G, Ls, L), A)
