"""The fused Adam kernels (csrc/optim.hip k_adam; the tails k_tf_tail / k_tf8_tail, which share common.h adam_elem) and the
receiver schedule (k_pick_rows) on the MI355X, called directly and pinned to an independent float64 Adam
(tests/adam_ref.py).  The criterion everywhere: per buffer (p, m, v) and step, the kernel's max / median absolute error
against float64 stays below twice that of torch.optim.Adam on float32 CPU copies of the same inputs.

Measured on the MI355X, worst kernel / torch-float32 error ratio per buffer (bound 2; 690 comparisons, none above 1.09):
  k_adam       p  max 1.09 (n = 26000, t = 1)   median 1.01 (n = 1023, t = 3)
               m  max 1.00                      median 1.00 (every size and step: torch's own bits)
               v  max 1.00 (n = 1, t = 1)       median 1.00 (n = 1, t = 1; 0.33 .. 0.82 at the other sizes)
  k_tf_tail    p 1.00 / 1.00   m 1.00 / 1.00   v max 1.00 (n = 2, t = 1), median 0.91 (n = 2, t = 2)
  k_tf8_tail   p 1.00 / 1.01   m 1.00 / 1.00   v max 1.00 (n = 5, t = 2), median 0.73 (n = 5, t = 2)
  step_range   p, m 1.00 / 1.00, v 0.46 / 0.61;   graph replay   p 1.00 / 1.01, m 1.00 / 1.00, v 0.97 (t = 2) / 0.45
History of the figures for v: with 1 - beta and the bias corrections formed in float from the rounded betas (1 - 0.999f is
1.3e-5 off) a float32 restatement of the kernel (tests/test_adam_ref.py) put m up to 16 and v up to 300 times torch's error
from float64 Adam, max and median alike.  With the constants from the double betas (common.h adam_consts) but v still
formed in float -- (g g)(1 - b2) fused into the add, three roundings on top of float(0.001)'s 4.7e-8 -- the medians sat at
1.0 .. 1.09 but the max, taken on the handful of elements with the largest |g| where either side is 0 .. 1.8 ulp off, missed
the bound in 8 comparisons (k_adam n = 1025: 2.94, n = 16384: 3.47; k_tf_tail n = 2: 2.67; k_tf8_tail n = 5: 2.65, all at
t = 1).  adam_elem now forms v in double and rounds once: at most half an ulp per step."""
import functools

import numpy as np
import pytest
import torch

from tests.adam_ref import adam_ref, check_against_float64, torch_adam32
from tests.margins import within

pytestmark = pytest.mark.gpu
DEV = "cuda"
BETAS, EPS = (0.9, 0.999), 1e-8
GUARD = 0x7FC12345            # a quiet-NaN bit pattern: a guard float that is read poisons what reads it
SIZES = [1, 1023, 1025, 16384, 16385, 26000, 512 * 2048, 512 * 2048 + 2049]

@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffgfdn_amd import hip_ops
    return hip_ops


# ---- inputs, drawn on the CPU -------------------------------------------------------------------------------------------
def _segments(n, rng):
    """uint8 group of every element: up to 255 contiguous groups whose boundaries are no multiple of 256 (so of no block
    or tile size), at least one group of a single element where n allows"""
    if n < 2000:
        return np.sort(rng.integers(0, 255, n)).astype(np.uint8)
    x = 1 + int(rng.integers(0, n - 8))
    x += 1 if (x % 256 == 0 or (x + 1) % 256 == 0) else 0
    x += 1 if (x % 256 == 0 or (x + 1) % 256 == 0) else 0
    cuts = {x, x + 1}                                       # the group [x, x + 1)
    while len(cuts) < 254:
        c = int(rng.integers(1, n))
        if c % 256:
            cuts.add(c)
    cuts = np.array(sorted(cuts))
    assert cuts.size == 254 and not (cuts % 256 == 0).any()
    seg = np.searchsorted(cuts, np.arange(n), side="right")
    assert np.bincount(seg).min() == 1
    return seg.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _case(n):
    """Inputs of one size and what float64 Adam and float32 torch make of them (computed once, read-only): steps 1, 2, 3 from
    zero moments, then one step from t = 999 with random moments.  Stretches: gradient always zero (moments zero too in its
    first half at t = 999), gradient zero on every third step; the last element's |g| = 1e-25 (g g underflows in float32);
    the group of element n // 3 has lr = 0."""
    f32 = np.float32
    rng = np.random.default_rng(1000 + n)
    seg = _segments(n, rng)
    lrs = [float(x) for x in 10.0 ** rng.uniform(-4, -1, 255)]
    scale = 10.0 ** rng.uniform(-12, 2, n)
    p0 = rng.standard_normal(n).astype(f32)
    grads = [(rng.standard_normal(n) * scale).astype(f32) for _ in range(4)]
    m999 = (0.5 * rng.standard_normal(n) * scale).astype(f32)
    v999 = ((rng.standard_normal(n) * scale) ** 2).astype(f32)
    c = dict(n=n, zero=slice(0, 0), third=slice(0, 0), frozen=np.zeros(n, bool))
    if n >= 8:
        w = max(1, n // 16)
        c['zero'], c['third'] = slice(n // 5, n // 5 + w), slice(n // 2, n // 2 + w)
        for g in grads:
            g[c['zero']] = 0.0
            g[n - 1] = f32(1e-25) * (1 if g[n - 1] >= 0 else -1)
        grads[2][c['third']] = 0.0
        still = slice(n // 5, n // 5 + (w + 1) // 2)
        m999[still] = 0.0
        v999[still] = 0.0
        c['still'] = still
        lrs[int(seg[n // 3])] = 0.0
        c['frozen'] = seg == seg[n // 3]
    z = np.zeros(n)
    c.update(seg=seg, lrs=lrs, p0=p0, grads=grads, m999=m999, v999=v999)
    c['ref'] = adam_ref(p0, z, z, grads[:3], lrs, seg, 0) + adam_ref(p0, m999, v999, grads[3:], lrs, seg, 999)
    c['yard'] = torch_adam32(p0, z, z, grads[:3], lrs, seg, 0) + torch_adam32(p0, m999, v999, grads[3:], lrs, seg, 999)
    for a in [seg, p0, m999, v999] + grads + [x for tup in c['ref'] + c['yard'] for x in tup]:
        a.setflags(write=False)
    return c


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _guarded(a):
    """a float32 array on the device with 64 guard floats on each side, inside one allocation: (allocation, view)"""
    buf = torch.empty(a.size + 128, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(GUARD)
    buf[64:64 + a.size].copy_(torch.from_numpy(np.array(a)))
    return buf, buf[64:64 + a.size]


def _guards_intact(buf):
    bits = buf.view(torch.int32)
    return bool((bits[:64] == GUARD).all()) and bool((bits[-64:] == GUARD).all())


def _host(*ts):
    return tuple(t.detach().cpu().numpy().reshape(-1) for t in ts)


# ---- 2. k_adam against float64, through the three entry points ---------------------------------------------------------------
@pytest.mark.parametrize("entry", ["plain", "counted", "mirrored"])
@pytest.mark.parametrize("n", SIZES)
def test_adam_step_against_float64(ops, n, entry):
    """hip_ops.adam_step on hand-built flat buffers: the single-block launch (n <= 16384), the multi-block launch with a
    ragged last block, the grid-stride loop with a second, ragged trip (n > 512 * 2048); without a block counter (separate
    advance launch), with one, and with the mirror.  After every launch: the counter(s) hold t exactly, the block counter is
    re-armed, lr_seg / seg / g are untouched, the guards around p, m, v are intact, p / m / v meet the criterion; where
    lr = 0 the parameters keep their bits while m, v move; where g, m, v are all zero p keeps its bits."""
    c = _case(n)
    seg, lr_seg = _dev(c['seg']), torch.tensor(c['lrs'], dtype=torch.float32).to(DEV)
    cnt = torch.zeros(1, dtype=torch.float32, device=DEV)
    mirror = torch.full((1,), -7.0, dtype=torch.float32, device=DEV) if entry == "mirrored" else None
    blk = torch.zeros(1, dtype=torch.int32, device=DEV) if entry != "plain" else None
    pbuf, p = _guarded(c['p0'])
    mbuf, m = _guarded(np.zeros(n, np.float32))
    vbuf, v = _guarded(np.zeros(n, np.float32))
    seg0, lr0 = seg.clone(), lr_seg.clone()
    for k, t in enumerate((1, 2, 3, 1000)):
        if t == 1000:
            p.copy_(_dev(c['p0']))
            m.copy_(_dev(c['m999']))
            v.copy_(_dev(c['v999']))
            cnt.fill_(999.0)
            if mirror is not None:
                mirror.fill_(999.0)
        g = _dev(c['grads'][k])
        g0, p_before = g.clone(), p.clone()
        ops.adam_step(p, g, m, v, seg, lr_seg, cnt, BETAS[0], BETAS[1], EPS, blk, mirror=mirror)
        torch.cuda.synchronize()
        label = f"k_adam[{entry}] n={n} t={t}"
        assert float(cnt) == float(t), label
        assert mirror is None or float(mirror) == float(t), label
        assert blk is None or int(blk) == 0, label
        assert torch.equal(g, g0) and torch.equal(seg, seg0) and torch.equal(lr_seg, lr0), label
        assert _guards_intact(pbuf) and _guards_intact(mbuf) and _guards_intact(vbuf), label
        got = _host(p, m, v)
        check_against_float64(got, c['yard'][k], c['ref'][k], label, within)
        fz = c['frozen']
        if fz.any():
            assert np.array_equal(got[0][fz].view(np.int32), _host(p_before)[0][fz].view(np.int32)), label
            moving = fz & (c['grads'][k] != 0)
            assert moving.any() and (got[1][moving] != 0).all(), label
            assert (got[2][moving & (np.abs(c['grads'][k]) > 1e-15)] > 0).all(), label
            z = c['zero'] if t != 1000 else c['still']         # gradient and both moments zero: 0 / (0 + eps)
            assert np.array_equal(got[0][z].view(np.int32), c['p0'][z].view(np.int32)), label
            assert not got[1][z].any() and not got[2][z].any(), label
            assert np.isfinite(got[0][n - 1]) and got[2][n - 1] >= 0.0, label


# ---- 3. a ranged step writes only its range ----------------------------------------------------------------------------------
def _leaves(sizes, gen):
    return [torch.nn.Parameter(torch.randn(k, generator=gen).to(DEV)) for k in sizes]


def _flat_adam(leaves, lrs):
    from diffgfdn_amd.optim import FlatAdam
    return FlatAdam([{'params': [q], 'lr': lr} for q, lr in zip(leaves, lrs)], betas=BETAS, eps=EPS)


def _fresh_grad(opt, gen):
    n = opt.flat_grad.numel()
    g = torch.randn(n, generator=gen) * 10.0 ** (14.0 * torch.rand(n, generator=gen) - 12.0)
    opt.flat_grad.copy_(g)
    opt._packed = True
    return g.numpy()


@pytest.mark.parametrize("lo,hi,second", [(1001, 1001 + 9000, False), (3001, 3001 + 20001, True)])
def test_step_range_writes_only_its_range(ops, lo, hi, second):
    """FlatAdam.step_range hands the kernel element-offset slices (odd ``lo``: 4-byte aligned pointers only), one range for
    the single-block launch and one for the multi-block launch: after a whole step (so that moments and counters are not
    zero) the ranged step leaves every bit outside [lo, hi) of flat_param / exp_avg / exp_avg_sq and the counter it does
    not own alone, advances its own, and the inside meets the criterion."""
    gen = torch.Generator(device="cpu").manual_seed(lo)
    sizes, lrs = (4999, 7001, 13, 18000), (1e-2, 3e-3, 0.0, 1e-3)
    opt = _flat_adam(_leaves(sizes, gen), lrs)
    _fresh_grad(opt, gen)
    opt.step()
    g2 = _fresh_grad(opt, gen)
    torch.cuda.synchronize()
    before = _host(opt.flat_param, opt.exp_avg, opt.exp_avg_sq)
    seg = opt.seg.cpu().numpy()
    opt.step_range(lo, hi, second=second)
    torch.cuda.synchronize()
    after = _host(opt.flat_param, opt.exp_avg, opt.exp_avg_sq)
    own, other = (opt.step_count2, opt.step_count) if second else (opt.step_count, opt.step_count2)
    assert float(own) == 2.0 and float(other) == 1.0
    assert int(opt._block_counter) == 0 and int(opt._block_counter2) == 0
    outside = np.ones(seg.size, bool)
    outside[lo:hi] = False
    for a, b in zip(after, before):
        assert np.array_equal(a[outside].view(np.int32), b[outside].view(np.int32))
    sl = slice(lo, hi)
    ins = [b[sl] for b in before]
    ref = adam_ref(*ins, [g2[sl]], lrs, seg[sl], 1, BETAS, EPS)
    yard = torch_adam32(*ins, [g2[sl]], lrs, seg[sl], 1, BETAS, EPS)
    check_against_float64([a[sl] for a in after], yard[0], ref[0], f"step_range [{lo}, {hi}) t=2", within)


# ---- 4. split step on two streams == the whole step, at the bank's size ------------------------------------------------------------
def test_split_step_on_two_streams_equals_the_whole_step():
    """Two FlatAdam over the same leaves (26 003 floats in four groups, the last the gain network's range): A steps whole, B
    steps [0, w_lo) and [w_lo, n) from two streams ordered by events as bankstep.py does (w_lo odd; 8 003 elements for the
    single-block launch, 18 000 for the multi-block one).  Three steps: parameters and both moments bit for bit, all four
    counters at the step number, both block counters re-armed; then one unsplit step of B (the mirror kept them equal)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    gen = torch.Generator(device="cpu").manual_seed(77)
    sizes, lrs = (2500, 2503, 3000, 18000), (1e-2, 1e-2, 1e-3, 3e-3)
    init = _leaves(sizes, gen)
    opt_a = _flat_adam([torch.nn.Parameter(q.detach().clone()) for q in init], lrs)
    opt_b = _flat_adam([torch.nn.Parameter(q.detach().clone()) for q in init], lrs)
    n = opt_b.flat_param.numel()
    w_lo = opt_b.flat_range(opt_b._params[3])[0]
    assert w_lo % 2 == 1 and w_lo < 16384 < n - w_lo
    main, s1, s2 = torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()
    for step in range(1, 5):
        g = _fresh_grad(opt_a, gen)
        opt_b.flat_grad.copy_(torch.from_numpy(g))
        opt_b._packed = True
        opt_a.step()
        if step < 4:
            ready = torch.cuda.Event()
            ready.record()                       # the gradients are complete on the main stream
            with torch.cuda.stream(s1):
                s1.wait_event(ready)
                opt_b.step_range(0, w_lo, second=False)
            with torch.cuda.stream(s2):
                s2.wait_event(ready)
                opt_b.step_range(w_lo, n, second=True)
            main.wait_stream(s1)
            main.wait_stream(s2)
        else:
            opt_b._packed = True
            opt_b.step()
        torch.cuda.synchronize()
        for a, b in ((opt_a.flat_param, opt_b.flat_param), (opt_a.exp_avg, opt_b.exp_avg),
                     (opt_a.exp_avg_sq, opt_b.exp_avg_sq)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), step
        for cnt in (opt_a.step_count, opt_a.step_count2, opt_b.step_count, opt_b.step_count2):
            assert float(cnt) == float(step), step
        for blk in (opt_a._block_counter, opt_a._block_counter2, opt_b._block_counter, opt_b._block_counter2):
            assert int(blk) == 0, step


# ---- 5. replay from a captured graph ---------------------------------------------------------------------------------------------
def test_step_replayed_from_a_graph_against_float64():
    """opt.step() captured once on a single stream (after a warm-up step, gradients written into flat_grad between replays)
    and replayed four times, one group's learning rate halved through param_groups + sync_lr() between the second and the
    third replay (what StepLR does in the trainers): the device counter advances by one per replay and p, m, v meet the
    criterion after every replay against adam_ref given the changed rate from then on."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    gen = torch.Generator(device="cpu").manual_seed(55)
    sizes = (3001, 2999, 2000, 18000)
    lrs = [1e-2, 3e-3, 1e-3, 2e-3]
    leaves = _leaves(sizes, gen)
    p0 = np.concatenate(_host(*leaves))
    opt = _flat_adam(leaves, lrs)
    assert opt.flat_param.numel() == 26000
    seg = opt.seg.cpu().numpy()
    grads = [_fresh_grad(opt, gen)]
    opt.step()                                   # warm-up
    opt._packed = True
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert float(opt.step_count) == 1.0          # (a capture runs nothing)
    rows, states = [list(lrs)], [_host(opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
    for r in range(4):
        if r == 2:
            opt.param_groups[1]['lr'] = 0.5 * opt.param_groups[1]['lr']
            opt.sync_lr()
        rows.append([float(g['lr']) for g in opt.param_groups])
        grads.append(_fresh_grad(opt, gen))
        graph.replay()
        torch.cuda.synchronize()
        assert float(opt.step_count) == r + 2.0 and float(opt.step_count2) == r + 2.0, r
        assert int(opt._block_counter) == 0, r
        states.append(_host(opt.flat_param, opt.exp_avg, opt.exp_avg_sq))
    assert rows[3][1] == 0.5 * lrs[1] and rows[2] == lrs
    z = np.zeros(p0.size)
    ref = adam_ref(p0, z, z, grads, rows, seg, 0, BETAS, EPS)
    yard = torch_adam32(p0, z, z, grads, rows, seg, 0, BETAS, EPS)
    for k, got in enumerate(states):
        check_against_float64(got, yard[k], ref[k], f"graph replay n=26000 t={k + 1}", within)
    del graph


# ---- 6. the tails: equal to the separate launches bit for bit, and pinned to float64 ---------------------------------------------
def _bank_blocks(gen, nblk, n):
    M = (torch.randn(nblk, n, n, generator=gen) / np.sqrt(n)).to(DEV)
    b = (torch.randn(nblk * n, generator=gen) / n).to(DEV)
    c = (torch.randn(nblk * n, generator=gen) / n).to(DEV)
    ig = (1.0 + 0.01 * torch.rand(nblk * n, generator=gen)).to(DEV)
    return M, b, c, ig


@pytest.mark.parametrize("n", [8, 6, 5, 4, 3, 2])
def test_fused_tails_equal_separate_launches_and_float64(ops, n):
    """n > 4: gfdn_tf8_tail == gfdn_tf8_param_grads, then FlatAdam.step(), then gfdn_ortho_fwd of the updated blocks (the
    small-shape twin of test_gpu_round5.test_fused_tail_equals_separate_launches, which does the same for gfdn_tf_tail and
    gfdn_tf_ortho_coefs: n <= 4 here): gradients, parameters, both moments, both counters and the next step's Q / Q Q /
    gain snapshot (record sets), two steps in a row, bit for bit -- and the fused side's parameters and moments against
    adam_ref fed the gradients of the separate launches, so that the tails hang on float64 Adam and not only on k_adam."""
    from diffgfdn_amd.optim import FlatAdam
    gen = torch.Generator(device="cpu").manual_seed(140 + n)
    nblk, parts, big = 6, 9, n > 4
    M0, b0, c0, ig = _bank_blocks(gen, nblk, n)
    lrs = (1e-2, 1e-2, 1e-3, 1e-2)

    def build():
        c = torch.nn.Parameter(c0.clone())
        b = torch.nn.Parameter(b0.clone())
        M = torch.nn.Parameter(M0.clone())
        w = torch.nn.Parameter(torch.zeros(5, device=DEV))
        opt = FlatAdam([{'params': [q], 'lr': lr} for q, lr in zip((c, b, M, w), lrs)], betas=BETAS, eps=EPS)
        return opt, M, b, c

    def records(M, b, c, out=None):
        if not big:
            return ops.tf_ortho_coefs(M.data, ig, b.data, c.data, out=out)
        Q, QQ = ops.ortho_fwd(M.data, True, True)
        return Q, QQ, c.data.clone()

    opt_a, Ma, ba, ca = build()
    opt_b, Mb, bb, cb = build()
    rec_b = tuple(t.clone() for t in records(Mb, bb, cb))
    offs = (opt_b.flat_range(Mb)[0], opt_b.flat_range(bb)[0], opt_b.flat_range(cb)[0])
    views = {id(p): v for p, v in zip(opt_b._params, opt_b._grad_views)}
    va = {id(p): v for p, v in zip(opt_a._params, opt_a._grad_views)}
    seg = opt_a.seg.cpu().numpy()
    for step in range(2):
        rows = 512 if big else 32
        grec0 = torch.randn(nblk, rows, parts, generator=gen).to(DEV)
        grec1 = (torch.randn(nblk, rows, parts, generator=gen) if big else torch.randn(nblk, rows, generator=gen)).to(DEV)
        gQ = torch.randn(nblk, n, n, generator=gen).to(DEV)
        before = _host(opt_a.flat_param, opt_a.exp_avg, opt_a.exp_avg_sq)
        # separate launches
        Qa, QQa = records(Ma, ba, ca)[:2]
        if big:
            ops.tf8_param_grads(QQa, ig, grec0, ba.data, ca.data, Ma.data, A1=Ma.data, part1=grec1, gQ=gQ, Q=Qa,
                                gb=va[id(ba)].view(-1), gc=va[id(ca)].view(-1), gM=va[id(Ma)])
        else:
            ops.tf_param_grads(QQa, ig, grec0, ba.data, ca.data, Ma.data, A1=Ma.data, grec1=grec1, gQ=gQ, Q=Qa,
                               gb=va[id(ba)].view(-1), gc=va[id(ca)].view(-1), gM=va[id(Ma)])
        opt_a._packed = True
        opt_a.step()
        rec_a = records(Ma, ba, ca)
        # the fused launch (the gradient of the fourth leaf is zero: its range is stepped by the plain kernel)
        Qb, QQb = rec_b[0], rec_b[1]
        if big:
            ops.tf8_tail(QQb, ig, grec0, grec1, bb.data, cb.data, Mb.data.view(nblk, n, n), gQ, Qb, views[id(bb)].view(-1),
                         views[id(cb)].view(-1), views[id(Mb)], opt_b, *offs, *rec_b)
        else:
            ops.tf_tail(QQb, ig, grec0, grec1, bb.data, cb.data, Mb.data.view(nblk, n, n), gQ, Qb, views[id(bb)].view(-1),
                        views[id(cb)].view(-1), views[id(Mb)].view(-1), opt_b, *offs, *rec_b)
        opt_b.step_range(opt_b.flat_range(opt_b._params[3])[0], opt_b.flat_grad.numel(), second=True)
        torch.cuda.synchronize()
        assert torch.equal(opt_a.flat_grad, opt_b.flat_grad), step
        assert torch.equal(opt_a.flat_param, opt_b.flat_param), step
        assert torch.equal(opt_a.exp_avg, opt_b.exp_avg) and torch.equal(opt_a.exp_avg_sq, opt_b.exp_avg_sq), step
        assert float(opt_a.step_count) == step + 1 and float(opt_a.step_count2) == step + 1
        assert float(opt_b.step_count) == step + 1 and float(opt_b.step_count2) == step + 1
        assert int(opt_b._block_counter) == 0 and int(opt_b._block_counter2) == 0
        assert len(rec_a) == len(rec_b)
        for got, want in zip(rec_b, rec_a):
            assert torch.equal(got, want), step
        g = _host(opt_a.flat_grad)[0]
        assert np.abs(g[:-5]).min() > 0.0 and not g[-5:].any()
        ref = adam_ref(*before, [g], lrs, seg, step, BETAS, EPS)
        yard = torch_adam32(*before, [g], lrs, seg, step, BETAS, EPS)
        check_against_float64(_host(opt_b.flat_param, opt_b.exp_avg, opt_b.exp_avg_sq), yard[0], ref[0],
                              f"{'k_tf8_tail' if big else 'k_tf_tail'} n={n} t={step + 1}", within)


# ---- 7. the receiver schedule ----------------------------------------------------------------------------------------------------
GUARD64 = 0x5A5A5A5A5A5A5A5A


def _schedule(B, length, pos0, state_len, gen):
    table = torch.randint(0, 1 << 40, (length, B), generator=gen, dtype=torch.long)
    buf = torch.full((B + 64,), GUARD64, dtype=torch.long, device=DEV)
    state = torch.tensor([pos0, state_len], dtype=torch.long, device=DEV)
    return table, table.to(DEV), buf, buf[:B], state


@pytest.mark.parametrize("B", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("length,pos0,state_len", [(1, 0, 1), (3, 0, 3), (3, 2, 3), (3, (1 << 33) + 1, 3), (3, 5, 0),
                                                   (3, 4, -2)])
def test_pick_rows_against_integer_indexing(ops, B, length, pos0, state_len):
    """hip_ops.pick_rows called directly, len + 2 times in a row (the position wraps): idx == table[pos % len] exactly, the
    position advances by one, the length, the table and a guard behind idx inside the same allocation are untouched; the
    loop over B > 256; a position above 2^33 (64-bit arithmetic: its low 32 bits name another row); len <= 0 in the state
    reads row 0 every time (the kernel's guard: no division by zero)."""
    gen = torch.Generator(device="cpu").manual_seed(B + 7 * length)
    table, table_d, buf, idx, state = _schedule(B, length, pos0, state_len, gen)
    eff = state_len if state_len > 0 else 1
    assert pos0 < (1 << 32) or (pos0 % eff) != ((pos0 & 0xFFFFFFFF) % eff)
    for k in range(length + 2):
        out = ops.pick_rows(table_d, state, idx)
        torch.cuda.synchronize()
        assert out is idx
        assert torch.equal(idx.cpu(), table[(pos0 + k) % eff]), k
        assert state.cpu().tolist() == [pos0 + k + 1, state_len], k
        assert bool((buf[B:] == GUARD64).all()) and torch.equal(table_d.cpu(), table), k


@pytest.mark.parametrize("B,length", [(257, 3), (4, 1)])
def test_pick_rows_replayed_from_a_graph(ops, B, length):
    """one launch captured in a single-stream graph and replayed len + 1 times: the schedule advances per replay"""
    gen = torch.Generator(device="cpu").manual_seed(B)
    table, table_d, buf, idx, state = _schedule(B, length, 0, length, gen)
    ops.pick_rows(table_d, state, idx)           # warm-up: position 0 -> 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.pick_rows(table_d, state, idx)
    for k in range(1, length + 2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(idx.cpu(), table[k % length]), k
        assert state.cpu().tolist() == [k + 1, length], k
        assert bool((buf[B:] == GUARD64).all()), k
    del graph
