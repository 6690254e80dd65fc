"""tests/adam_ref.py checked before the GPU tests lean on it: the float64 reference against torch.optim.Adam on float64 CPU
tensors, and what the criterion says about a numpy float32 restatement of the kernel's pinned roundings (common.h
adam_elem) with its constants formed from the double betas and from their float roundings."""
import numpy as np
import torch

from tests.adam_ref import adam_ref, error_bounds, torch_adam32


def test_adam_ref_equals_torch_float64():
    """three param groups, 5 steps, foreach=False, an element whose gradient is always zero: 1e-12 relative"""
    rng = np.random.default_rng(3)
    sizes, lrs = (7, 1, 12), (1e-3, 3e-2, 7e-4)
    n = sum(sizes)
    seg = np.repeat(np.arange(3), sizes)
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n) for _ in range(5)]
    for g in grads:
        g[3] = 0.0
    ref = adam_ref(p0, np.zeros(n), np.zeros(n), grads, lrs, seg, 0)
    off = np.concatenate(([0], np.cumsum(sizes)))
    params = [torch.nn.Parameter(torch.tensor(p0[a:b], dtype=torch.float64)) for a, b in zip(off[:-1], off[1:])]
    opt = torch.optim.Adam([{'params': [q], 'lr': lr} for q, lr in zip(params, lrs)], betas=(0.9, 0.999), eps=1e-8,
                           foreach=False)
    for k, g in enumerate(grads):
        for q, a, b in zip(params, off[:-1], off[1:]):
            q.grad = torch.tensor(g[a:b], dtype=torch.float64)
        opt.step()
        want = (np.concatenate([q.detach().numpy() for q in params]),
                np.concatenate([opt.state[q]['exp_avg'].numpy() for q in params]),
                np.concatenate([opt.state[q]['exp_avg_sq'].numpy() for q in params]))
        for name, got, w in zip("pmv", ref[k], want):
            assert np.abs(got - w).max() <= 1e-12 * np.abs(w).max(), (k, name)
    assert ref[4][0][3] == p0[3] and ref[4][1][3] == 0.0 and ref[4][2][3] == 0.0


def test_adam_ref_starts_anywhere_and_takes_a_learning_rate_per_step():
    """t0 > 0 with given moments == the tail of a run from 0; a row of learning rates per gradient"""
    rng = np.random.default_rng(4)
    n = 9
    seg = np.repeat(np.arange(3), 3)
    lrs = [1e-2, 0.0, 1e-3]
    grads = [rng.standard_normal(n) for _ in range(4)]
    p0 = rng.standard_normal(n)
    whole = adam_ref(p0, np.zeros(n), np.zeros(n), grads, [lrs, lrs, [0.5 * lr for lr in lrs], lrs], seg, 0)
    rest = adam_ref(*whole[1], grads[2:], [[0.5 * lr for lr in lrs], lrs], seg, 2)
    for a, b in zip(whole[3], rest[1]):
        assert np.array_equal(a, b)
    assert np.array_equal(whole[3][0][3:6], p0[3:6]) and np.abs(whole[3][1][3:6]).min() > 0.0


def _kernel_arithmetic32(p, g, m, v, lr, t, consts):
    """common.h adam_elem / adam_bias_corr in numpy float32 (the fused multiply-add through float64: the product is exact
    there; the second moment in float64, rounded once, as the kernel forms it)"""
    f32, f64 = np.float32, np.float64
    omb1, b2, omb2, lb1, lb2, eps = consts
    bc1 = f32(-np.expm1(f64(f32(t) * lb1)))
    bc2_sqrt = np.sqrt(f32(-np.expm1(f64(f32(t) * lb2))))
    m = ((g - m).astype(f64) * f64(omb1) + m.astype(f64)).astype(f32)
    v = (g.astype(f64) * g.astype(f64) * f64(omb2) + v.astype(f64) * f64(b2)).astype(f32)
    denom = np.sqrt(v) / bc2_sqrt + eps
    return (p - (lr / bc1) * (m / denom)).astype(f32), m, v


def test_constants_formed_from_the_rounded_betas_miss_the_criterion_by_far():
    """Why the kernels take the betas as doubles: with 1 - beta and the bias corrections formed in float from the ROUNDED
    betas (1 - 0.9f is 2.4e-7 off, 1 - 0.999f 1.3e-5) the moments' median error against float64 Adam is tens to hundreds of
    times float32 torch's; formed from the doubles (common.h adam_consts) it is torch's own.  (The max figures of the
    criterion hang on the few elements of the top binade, where the two sides' different rounding orders decide: not
    judged here.)"""
    f32 = np.float32
    rng = np.random.default_rng(5)
    n = 4096
    seg = np.sort(rng.integers(0, 255, n))
    lrs = 10.0 ** rng.uniform(-4, -1, 255)
    p0 = rng.standard_normal(n).astype(f32)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-12, 2, n)).astype(f32) for _ in range(3)]
    z = np.zeros(n)
    ref = adam_ref(p0, z, z, grads, lrs, seg, 0)
    yard = torch_adam32(p0, z, z, grads, lrs, seg, 0)
    b1, b2 = 0.9, 0.999
    good = (f32(1.0 - b1), b2, 1.0 - b2, f32(np.log(b1)), f32(np.log(b2)), f32(1e-8))
    bad = (f32(1) - f32(b1), f32(b2), f32(1) - f32(b2), f32(np.log(f32(b1))), f32(np.log(f32(b2))), f32(1e-8))
    for consts, is_good in ((good, True), (bad, False)):
        p, m, v, lr = p0, z.astype(f32), z.astype(f32), lrs.astype(f32)[seg]
        for k in range(3):
            p, m, v = _kernel_arithmetic32(p, grads[k], m, v, lr, k + 1, consts)
            for name, got, y, r in zip("pmv", (p, m, v), yard[k], ref[k]):
                med = np.median(np.abs(got.astype(np.float64) - r))
                bound = error_bounds(y, r)[1]
                if is_good:
                    assert med < bound, (k, name, med, bound)
                elif name != "p":
                    assert med > 5.0 * bound, (k, name, med, bound)
