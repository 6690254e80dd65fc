"""An independent Adam for the optimiser tests: ``adam_ref`` is the formula in the header of csrc/optim.hip in plain numpy
float64 (no torch in the arithmetic); ``torch_adam32`` is the yardstick the GPU kernels are measured against, the reference
project's own optimiser (torch.optim.Adam, foreach=False, capturable=False) on float32 CPU copies of the same inputs;
``check_against_float64`` is the criterion: the kernel's error against float64 may be at most twice float32 torch's."""
import numpy as np

ERR_FACTOR = 2.0        # kernel error < ERR_FACTOR x float32 torch's error (max and median, per buffer)


def _lr_rows(lrs, steps):
    """(steps, groups) float64: one row of learning rates per step (``lrs``: one row for all steps, or one per step)"""
    a = np.asarray(lrs, dtype=np.float64)
    if a.ndim == 1:
        a = np.broadcast_to(a, (steps, a.shape[0]))
    if a.shape[0] != steps:
        raise ValueError("one row of learning rates per gradient")
    return a


def adam_ref(p, m, v, grads, lrs, seg, t0, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam without amsgrad / weight decay in float64:  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
    p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps), t = t0 + 1, t0 + 2, ... for each gradient in turn.
    ``seg[i]``: group of element i; ``lrs``: the groups' learning rates (Python doubles), or one such row per gradient.
    Returns [(p, m, v) after each step]."""
    p, m, v = (np.array(a, dtype=np.float64) for a in (p, m, v))
    seg = np.asarray(seg).astype(np.int64)
    b1, b2 = float(betas[0]), float(betas[1])
    rows = _lr_rows(lrs, len(grads))
    out = []
    for k, g in enumerate(grads):
        g = np.asarray(g, dtype=np.float64)
        t = int(t0) + k + 1
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        lr = rows[k][seg]
        p = p - lr / (1.0 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
        out.append((p.copy(), m.copy(), v.copy()))
    return out


def _runs(seg):
    """[(group, lo, hi)] of a segment map whose groups are contiguous runs"""
    seg = np.asarray(seg).astype(np.int64)
    cut = np.flatnonzero(np.diff(seg)) + 1
    lo = np.concatenate(([0], cut))
    hi = np.concatenate((cut, [seg.size]))
    runs = [(int(seg[a]), int(a), int(b)) for a, b in zip(lo, hi)]
    if len({g for g, _, _ in runs}) != len(runs):
        raise ValueError("every group must be one contiguous run")
    return runs


def torch_adam32(p, m, v, grads, lrs, seg, t0, betas=(0.9, 0.999), eps=1e-8):
    """The same steps by torch.optim.Adam (foreach=False, capturable=False) on float32 CPU tensors, one parameter per
    group (the groups of ``seg`` must be contiguous runs).  Returns [(p, m, v) float32 arrays after each step]."""
    import torch
    runs = _runs(seg)
    rows = _lr_rows(lrs, len(grads))
    f32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))
    params = [torch.nn.Parameter(f32(p[lo:hi])) for _, lo, hi in runs]
    opt = torch.optim.Adam([{'params': [q], 'lr': float(rows[0][g])} for q, (g, _, _) in zip(params, runs)],
                           betas=tuple(betas), eps=eps, foreach=False, capturable=False)
    for q, (_, lo, hi) in zip(params, runs):
        opt.state[q] = {'step': torch.tensor(float(t0)), 'exp_avg': f32(m[lo:hi]), 'exp_avg_sq': f32(v[lo:hi])}
    out = []
    for k, g in enumerate(grads):
        for q, grp, (gi, lo, hi) in zip(params, opt.param_groups, runs):
            q.grad = f32(g[lo:hi])
            grp['lr'] = float(rows[k][gi])
        opt.step()
        cat = lambda ts: np.concatenate([t.detach().numpy().reshape(-1) for t in ts])
        out.append((cat(params), cat([opt.state[q]['exp_avg'] for q in params]),
                    cat([opt.state[q]['exp_avg_sq'] for q in params])))
        assert all(float(opt.state[q]['step']) == t0 + k + 1 for q in params)
    return out


def error_bounds(yard, ref):
    """(max bound, median bound) for one buffer: ERR_FACTOR x float32 torch's max / median absolute error against the
    float64 reference; where torch's own figure is 0, one float32 ulp of the buffer's largest magnitude stands in."""
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(np.asarray(yard, dtype=np.float64) - ref)
    ulp = float(np.spacing(np.float32(np.abs(ref).max()))) if ref.size else 0.0
    ulp = ulp if ulp > 0.0 else float(np.spacing(np.float32(0.0)))
    fig = lambda e: float(e) if float(e) > 0.0 else ulp
    return ERR_FACTOR * fig(err.max()), ERR_FACTOR * fig(np.median(err))


def check_against_float64(got, yard, ref, label, within, sel=None):
    """The criterion: for each of p, m, v the kernel's max (median) absolute error against float64 Adam stays below twice
    float32 torch's max (median).  ``got`` / ``yard`` / ``ref``: (p, m, v) of the kernel, of torch_adam32 and of adam_ref
    after the same step; ``sel``: the elements to judge (a slice or index array).  Every comparison goes through
    ``within`` (tests.margins.within); returns {buffer: (max ratio, median ratio)} against torch's figures."""
    ratios = {}
    for name, a, y, r in zip("pmv", got, yard, ref):
        a, y, r = (np.asarray(x).reshape(-1) for x in (a, y, r))
        if sel is not None:
            a, y, r = a[sel], y[sel], r[sel]
        assert np.isfinite(a).all(), (label, name, "not finite")
        err = np.abs(a.astype(np.float64) - r)
        bmax, bmed = error_bounds(y, r)
        within(err.max(), bmax, f"{label} {name} max")
        within(np.median(err), bmed, f"{label} {name} median")
        ratios[name] = (ERR_FACTOR * err.max() / bmax, ERR_FACTOR * float(np.median(err)) / bmed)
    return ratios
