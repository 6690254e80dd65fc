"""Plain float64 numpy restatement of the reference's moving-listener render
(sound_examples.py:163-226 ``dynamic_rendering_moving_receiver.filter_overlap_add``), pinned to the reference's own output by
``tests/test_moving_listener_golden.py`` and the yardstick of ``tests/test_gpu_moving.py``.

    h = int(update_ms 1e-3 fs),  Fd = int(fade_len_ms 1e-3 fs),  total = P h
    x = the stimulus as float32, repeated or cut to total samples;  x_k = x[k h : (k + 1) h]
    f_0 = r_0,  f_k = alpha r_k + (1 - alpha) f_{k-1}                          (the recursion runs on the interpolated filter)
    s_k = (x_k * f_k)[: min(h + Lr - 1, total - k h)]
    out = OLA(s) + sum_{k >= 1} fade_out[i] (t_{k-1}[i] - s_k[i]) on [k h, k h + Fd),  t_{k-1} = the last Fd samples of s_{k-1}
"""
import numpy as np


def ms_to_samps(ms: float, fs: float) -> int:
    return int(ms * 1e-3 * fs)                                     # utils.py:62-80: truncation


def extended_stimulus(stimulus, total: int) -> np.ndarray:
    """sound_examples.py:149-161: float32, repeated or cut to ``total`` samples"""
    s = np.asarray(stimulus).astype(np.float32).reshape(-1)
    return np.tile(s, -(-total // s.size))[:total]


def fade_windows(Fd: int):
    n = np.linspace(-1.0, 1.0, Fd)
    return 0.5 * (1.0 + n), 0.5 * (1.0 - n)                         # (fade_in, fade_out), :118-127


def segments(rirs, path, x, h: int, alpha: float):
    """the cut segments s_k (float64) of the path"""
    rirs = np.asarray(rirs, dtype=np.float64)
    total = len(path) * h
    out, f = [], None
    for k, row in enumerate(path):
        f = rirs[row] if f is None else alpha * rirs[row] + (1.0 - alpha) * f
        s = np.convolve(x[k * h:(k + 1) * h].astype(np.float64), f)
        out.append(s[:min(s.size, total - k * h)])
    return out


def overlap_add(segs, h: int, Fd: int, branchy: bool = False) -> np.ndarray:
    """float64 (P h,).  ``branchy``: the reference's own loop (:199-224) instead of OLA + fade_out (t - s)"""
    total = len(segs) * h
    if not 1 <= Fd <= h:
        raise ValueError("1 <= Fd <= h")
    fade_in, fade_out = fade_windows(Fd)
    out = np.zeros(total)
    if branchy:
        prev_tail = np.zeros(Fd)
        for k, s in enumerate(segs):
            a = k * h
            if k > 0:
                n = min(Fd, s.size)
                out[a:a + n] += prev_tail[:n] * fade_out[:n] + s[:n] * fade_in[:n]
                out[a + n:a + s.size] += s[n:]
            else:
                out[a:a + s.size] += s
            if s.size >= Fd:
                prev_tail[:Fd] = s[-Fd:]
            else:
                prev_tail[:s.size] = s
        return out
    for k, s in enumerate(segs):
        out[k * h:k * h + s.size] += s
        if k > 0:
            out[k * h:k * h + Fd] += fade_out * (segs[k - 1][-Fd:] - s[:Fd])
    return out


def ref_moving_listener(rirs, path, stimulus, fs: float, update_ms: float = 100.0, alpha: float = 0.5,
                        fade_len_ms: float = 50.0, branchy: bool = False) -> np.ndarray:
    path = [int(p) for p in path]
    h, Fd = ms_to_samps(update_ms, fs), ms_to_samps(fade_len_ms, fs)
    if not path or h < 1:
        raise ValueError("P >= 1 and h >= 1")
    x = extended_stimulus(stimulus, len(path) * h)
    return overlap_add(segments(rirs, path, x, h, alpha), h, Fd, branchy)
