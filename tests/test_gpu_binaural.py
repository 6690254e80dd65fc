"""Binaural render of a moving, head-turning listener (subband.render_binaural_moving_listener_bands /
render_binaural_moving_listener, csrc/binaural.hip) on the MI355X.

  1. ``binaural_compose`` against float64 (tests/binaural_ref.brtfs) on the same float32 inputs: nb = 512 (Kb = 257: an odd
     row length, a last workgroup with one live lane), P = 9 with repeats, (S, Ls) in {(1, 4), (7, 9), (32, 16)} and rows
     mode, alpha in {0.5, 1.0, 0.25}, pitched rows whose padding holds a sentinel; chunks of 4 + 4 + 1 with another pitch
     give the bits of the single launch; bad arguments are refused.
  2. ``binaural_ola`` against float64 (binaural_ref.overlap_add): h = 48, nb = 256, P = 9, Fd in {48, 24, 1}; chunks are
     bit-equal to the single launch; a sentinel behind the output is intact; tail_in == tail_out is refused.  (The kernel
     has no vector path: one sample of both ears per lane whatever h.)
  3. ``render_binaural_moving_listener`` against every case of tests/golden/f20_binaural.npz, inside CONVOLVE = 1e-5 of the
     largest output, the project's bar for one transform-product-transform convolution (test_gpu_moving.CONVOLVE).
  4. ``render_binaural_moving_listener_bands`` on small directional nets (Q = 3 bands of order 1 on K = 129, Q = 2 bands of
     order 2 on K = 257, G = 2) against binaural_ref in float64 on ``infer_directional_bands(.., directional=False,
     rows=path)``, inside PARITY = 1e-4; DirectionalBank.render_binaural; the fallback beyond the kernel's limits; errors.

The bounds of 1. and 2. are NOT 5e-6 by habit.  Measure: the same formula in float32 with stock tensor operations
(subband.binaural_compose_torch on float32 spectra; a float32 torch loop for the overlap-add) against the float64
restatement on the same inputs, error as a fraction of the largest output.  Stock float32 scores, printed by every run
([yardstick] lines): compose 0.68e-7 .. 2.58e-7 over the twelve cases (the kernel: 0.71e-7 .. 2.80e-7), overlap-add
4.7e-8 .. 7.9e-8 (the kernel: the same figures).  The bounds are 3 x the largest: COMPOSE = 8e-7, OLA = 2.4e-7."""
import numpy as np
import pytest
import torch

from tests import binaural_ref as bref
from tests.margins import within
from tests.test_binaural_golden import NUM_CASES, case, fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
COMPOSE, OLA, CONVOLVE, PARITY = 8e-7, 2.4e-7, 1e-5, 1e-4
SENTINEL = -12345.0
PATH = [3, 1, 1, 0, 4, 2, 3, 3, 1]
P, NB, KB, R = 9, 512, 257, 5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _frac(got, want):
    return float(np.abs(np.asarray(got, dtype=np.complex128) - want).max() / np.abs(want).max())


def _pitched_c(a: np.ndarray, pitch: int) -> torch.Tensor:
    """a (.., F) complex64 as the first F bins of a (.., pitch) device buffer; the padding holds SENTINEL"""
    buf = torch.full(a.shape[:-1] + (pitch,), SENTINEL, dtype=torch.complex64, device=DEV)
    buf[..., :a.shape[-1]] = torch.from_numpy(a).to(DEV)
    return buf


# ---- 1. compose -----------------------------------------------------------------------------------------------------
_problems = {}


def _problem(S, Ls):
    """inputs and the float64 spectra of a shape (S = 0: rows mode): computed once, shared by the cases, never written"""
    if (S, Ls) not in _problems:
        rng = np.random.RandomState(100 * S + Ls)
        cplx = lambda *s: (rng.randn(*s) + 1j * rng.randn(*s)).astype(np.complex64)        # noqa: E731
        p = dict(rot=rng.randn(P, Ls, Ls).astype(np.float32) / np.sqrt(Ls), Hh=cplx(Ls, 2, KB))
        if S:
            p["W"] = rng.randn(R, S, Ls).astype(np.float32)
            p["Ch"] = cplx(S * Ls, KB)
            store = np.einsum('rsm,smf->rmf', p["W"].astype(np.float64), p["Ch"].astype(np.complex128).reshape(S, Ls, KB))
        else:
            p["Ah"] = cplx(R, Ls, KB)
            store = p["Ah"].astype(np.complex128)
        p["A"] = store[PATH]
        _problems[(S, Ls)] = p
    return _problems[(S, Ls)]


def _compose(p, alpha, k0, nseg, pitch, out=None):
    from diffgfdn_amd import hip_ops as ops
    rot = torch.from_numpy(p["rot"]).to(DEV)
    Hh = _pitched_c(p["Hh"], pitch)
    path = torch.tensor(PATH, device=DEV)
    kw = dict(path=path, out=out)
    bufs = [Hh]
    if "W" in p:
        Ch = _pitched_c(p["Ch"], pitch)
        kw.update(W=torch.from_numpy(p["W"]).to(DEV), Ch=Ch[:, :KB])
        bufs.append(Ch)
    else:
        Ah = _pitched_c(p["Ah"], pitch)
        kw.update(Ah=Ah[:, :, :KB])
        bufs.append(Ah)
    got = ops.binaural_compose(rot, Hh[:, :, :KB], alpha, k0, nseg, **kw)
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[..., KB:] == SENTINEL).all())
    return got


@pytest.mark.parametrize("alpha", [0.5, 1.0, 0.25])
@pytest.mark.parametrize("S,Ls", [(1, 4), (7, 9), (32, 16), (0, 9)])
def test_compose_against_float64(S, Ls, alpha):
    from diffgfdn_amd.subband import binaural_compose_torch
    p = _problem(S, Ls)
    want = bref.brtfs(p["A"], p["rot"], p["Hh"], alpha)
    buf = torch.full((P, 2, KB + 3), SENTINEL, dtype=torch.complex64, device=DEV)
    got = _compose(p, alpha, 0, P, KB + 3, out=buf[:, :, :KB])
    assert got.data_ptr() == buf.data_ptr() and bool((buf[:, :, KB:] == SENTINEL).all())     # the padding survives
    # the yardstick: the same formula in float32, stock tensor operations, on the float32 store of the path's spectra
    A32 = torch.from_numpy(p["A"].astype(np.complex64)).to(DEV)
    stock = binaural_compose_torch(torch.from_numpy(p["rot"]).to(DEV), torch.from_numpy(p["Hh"]).to(DEV), alpha, 0, P, A32)
    print(f"[yardstick] compose S={S} Ls={Ls} alpha={alpha}: stock float32 {_frac(stock.cpu().numpy(), want):.3e}, "
          f"kernel {_frac(got.cpu().numpy(), want):.3e}")
    within(_frac(got.cpu().numpy(), want), COMPOSE, f"compose S={S} Ls={Ls} alpha={alpha}")
    # chunks of 4 + 4 + 1 and another pitch: the bits of the single launch
    parts = [_compose(p, alpha, k0, n, KB + 7) for k0, n in ((0, 4), (4, 4), (8, 1))]
    assert torch.equal(torch.cat(parts), got)


def test_compose_rows_without_path():
    """rows mode on a chunk's own store: row k - row_off, the store starting at segment k0 - 1"""
    from diffgfdn_amd import hip_ops as ops
    p = _problem(0, 9)
    full = _compose(p, 0.5, 0, P, KB)
    rot, Hh = torch.from_numpy(p["rot"]).to(DEV), torch.from_numpy(p["Hh"]).to(DEV)
    store = torch.from_numpy(p["Ah"][PATH[3:8]]).to(DEV)             # segments 3 .. 7
    got = ops.binaural_compose(rot, Hh, 0.5, 4, 4, Ah=store, row_off=3)
    assert torch.equal(got, full[4:8])


def test_compose_bad_arguments():
    from diffgfdn_amd import hip_ops as ops
    p = _problem(7, 9)
    rot, Hh = torch.from_numpy(p["rot"]).to(DEV), torch.from_numpy(p["Hh"]).to(DEV)
    W, Ch, Ah = torch.from_numpy(p["W"]).to(DEV), torch.from_numpy(p["Ch"]).to(DEV), torch.from_numpy(_problem(0, 9)["Ah"]).to(DEV)
    path = torch.tensor(PATH, device=DEV)
    ok = dict(W=W, Ch=Ch, path=path)
    ops.binaural_compose(rot, Hh, 0.5, 0, P, **ok)
    for bad in (dict(ok, W=None), dict(ok, Ch=None), dict(ok, Ah=Ah), dict(path=path), dict(ok, Ch=Ch[:-1]),
                dict(ok, W=W[:, :, :8]), dict(ok, path=path[:-1]), dict(ok, path=path + R), dict(ok, path=path.int()),
                dict(W=W, Ch=Ch), dict(ok, out=torch.empty((P, 2, KB), dtype=torch.float32, device=DEV)),
                dict(ok, out=torch.empty((P - 1, 2, KB), dtype=torch.complex64, device=DEV))):
        with pytest.raises(RuntimeError):
            ops.binaural_compose(rot, Hh, 0.5, 0, P, **bad)
    for k0, nseg, alpha in ((6, 4, 0.5), (-1, 2, 0.5), (0, 0, 0.5), (0, P, 1.5), (0, P, -0.1)):
        with pytest.raises(RuntimeError):
            ops.binaural_compose(rot, Hh, alpha, k0, nseg, **ok)
    with pytest.raises(RuntimeError):                                # the HRTFs of another channel count
        ops.binaural_compose(rot, Hh[:4], 0.5, 0, P, **ok)
    with pytest.raises(RuntimeError):                                # beyond the limits: no quiet fall-back here
        ops.binaural_compose(rot, Hh, 0.5, 0, P, W=torch.zeros(R, 33, 9, device=DEV),
                             Ch=torch.zeros(33 * 9, KB, dtype=torch.complex64, device=DEV), path=path)
    with pytest.raises(RuntimeError):
        ops.binaural_compose(rot.cpu(), Hh, 0.5, 0, P, **ok)


# ---- 2. overlap-add -------------------------------------------------------------------------------------------------
H, NB2, N2 = 48, 256, 512
LFULL = H + NB2 - 1

_ola = {}


def _ola_problem():
    if not _ola:
        rng = np.random.RandomState(2)
        s = (rng.randn(P, 2, N2) * np.exp(-np.arange(N2) / 150.0)).astype(np.float32)
        _ola.update(s=s, segs=[s[k].T.astype(np.float64)[:min(LFULL, (P - k) * H)] for k in range(P)])
    return _ola


def _ola_stock(s: torch.Tensor, Fd: int) -> torch.Tensor:
    """the reference's loop in float32 torch operations"""
    n = torch.linspace(-1.0, 1.0, Fd, device=DEV)
    fi, fo = torch.sqrt(0.5 * (1.0 + n))[:, None], torch.sqrt(0.5 * (1.0 - n))[:, None]
    out = torch.zeros((P * H, 2), device=DEV)
    for k in range(P):
        seg = s[k, :, :min(LFULL, (P - k) * H)].T
        if k:
            out[k * H:k * H + Fd] += tail * fo + seg[:Fd] * fi
            out[k * H + Fd:k * H + seg.shape[0]] += seg[Fd:]
        else:
            out[:seg.shape[0]] += seg
        tail = seg[-Fd:]
    return out


def _run_ola(s, Fd, chunks):
    from diffgfdn_amd import hip_ops as ops
    buf = torch.full((P * H + 8, 2), SENTINEL, device=DEV)
    out = buf[:P * H].zero_()
    tails = [torch.empty((Fd, 2), device=DEV) for _ in range(2)]
    k0 = 0
    for i, n in enumerate(chunks):
        ops.binaural_ola(s[k0:k0 + n], k0, P, H, NB2, Fd, out, tails[i & 1] if k0 else None, tails[1 - (i & 1)])
        k0 += n
    torch.cuda.synchronize()
    assert bool((buf[P * H:] == SENTINEL).all())                     # nothing behind the output
    return out


@pytest.mark.parametrize("Fd", [48, 24, 1])
def test_ola_against_float64(Fd):
    p = _ola_problem()
    want = bref.overlap_add(p["segs"], H, Fd)
    sbuf = torch.full((P, 2, N2 + 5), SENTINEL, device=DEV)          # (an odd pitch: the rows are read 4 bytes per lane)
    sbuf[:, :, :N2] = torch.from_numpy(p["s"]).to(DEV)
    got = _run_ola(sbuf[:, :, :N2], Fd, [P])
    assert bool((sbuf[:, :, N2:] == SENTINEL).all())
    print(f"[yardstick] ola Fd={Fd}: stock float32 {_frac(_ola_stock(sbuf[:, :, :N2], Fd).cpu().numpy(), want):.3e}, "
          f"kernel {_frac(got.cpu().numpy(), want):.3e}")
    within(_frac(got.cpu().numpy(), want), OLA, f"ola Fd={Fd}")
    s = torch.from_numpy(p["s"]).to(DEV)
    for chunks in ([4, 4, 1], [1] * P, [2, 7]):
        assert torch.equal(_run_ola(s, Fd, chunks), got), chunks


def test_ola_bad_arguments():
    from diffgfdn_amd import hip_ops as ops
    s = torch.from_numpy(_ola_problem()["s"]).to(DEV)
    out = torch.zeros((P * H, 2), device=DEV)
    t0, t1 = torch.empty((24, 2), device=DEV), torch.empty((24, 2), device=DEV)
    ops.binaural_ola(s[4:8], 4, P, H, NB2, 24, out, t0, t1)
    for args in ((s[4:8], 4, P, H, NB2, 24, out, t0, t0),            # tail_in is tail_out
                 (s[4:8], 4, P, H, NB2, 24, out, None, t1),          # no tail behind the first chunk
                 (s[4:8], 6, P, H, NB2, 24, out, t0, t1),            # segments 6 .. 9 of 9
                 (s[4:8], 4, P, H, NB2, 49, out, t0, t1), (s[4:8], 4, P, H, NB2, 0, out, t0, t1),
                 (s[4:8, :, :LFULL - 1], 4, P, H, NB2, 24, out, t0, t1),
                 (s[4:8, 0], 4, P, H, NB2, 24, out, t0, t1),
                 (s[4:8], 4, P, H, NB2, 24, out[:-1], t0, t1), (s[4:8], 4, P, H, NB2, 24, out.view(-1), t0, t1),
                 (s[4:8], 4, P, H, NB2, 24, out, t0[:, 0], t1)):
        with pytest.raises(RuntimeError):
            ops.binaural_ola(*args)


# ---- 3. the general function against the reference's own output -----------------------------------------------------
@pytest.mark.parametrize("i", range(NUM_CASES))
def test_render_against_the_golden_cases(i):
    from diffgfdn_amd.subband import render_binaural_moving_listener
    rirs, hrir, path, rot, stim, fs, update_ms, alpha, want = case(fixture(), i)
    got = render_binaural_moving_listener(rirs, hrir, path, rot, stim, fs, update_ms, alpha)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_cuda
    e = _frac(got.cpu().numpy(), want)
    print(f"[binaural] golden case {i}: {e:.3e} of the largest output")
    within(e, CONVOLVE, f"render golden case {i}")
    # a device tensor as the store and a buffer to fill: the same bits; chunks of 4: both kernels give the bits of one
    # launch, the stock complex product between them rounds by the batch's shape -- inside the same bound
    buf = torch.full(got.shape, SENTINEL, device=DEV)
    again = render_binaural_moving_listener(torch.from_numpy(rirs).to(DEV), hrir, path, rot, stim, fs, update_ms, alpha, out=buf)
    assert again.data_ptr() == buf.data_ptr() and torch.equal(again, got)
    parts = render_binaural_moving_listener(rirs, hrir, path, rot, stim, fs, update_ms, alpha, chunk=4)
    within(_frac(parts.cpu().numpy(), want), CONVOLVE, f"render golden case {i}, chunks of 4")


def test_render_path_none_and_many_channels():
    """path=None is every row in order; more than 16 channels take the stock-operations composition -- the same result as
    the kernel where both can run (Ls = 9 here, forced through it)"""
    from diffgfdn_amd import hip_ops as ops
    from diffgfdn_amd import subband
    rirs, hrir, path, rot, stim, fs, update_ms, alpha, _ = case(fixture(), 3)
    want = subband.render_binaural_moving_listener(rirs[path], hrir, list(range(len(path))), rot, stim, fs, update_ms, alpha)
    assert torch.equal(subband.render_binaural_moving_listener(rirs[path], hrir, None, rot, stim, fs, update_ms, alpha), want)
    keep = ops.BINAURAL_MAX_LS
    try:
        ops.BINAURAL_MAX_LS = 4
        stock = subband.render_binaural_moving_listener(rirs, hrir, path, rot, stim, fs, update_ms, alpha)
    finally:
        ops.BINAURAL_MAX_LS = keep
    within(_frac(stock.cpu().numpy(), want.cpu().numpy().astype(np.float64)), CONVOLVE, "stock composition")


# ---- 4. from the directional bands ----------------------------------------------------------------------------------
FS = 8000.0                                                           # update_ms = 6: h = 48


def _nets(Q, order, K, seed):
    """Q small directional nets (G = 2) as tests/test_gpu_parity._directional_bands builds them, freshly initialised"""
    from diffgfdn_amd.config import CouplingMatrixType, FeedbackLoopConfig, OutputFilterConfig
    from diffgfdn_amd.model import DiffDirectionalFDNVarReceiverPos
    G, Ls = 2, (order + 1) ** 2
    rng = np.random.RandomState(seed)
    delays = sorted(rng.choice(np.arange(37, 400), G * Ls, replace=False).tolist())
    A = rng.randn(Ls + 3, Ls).astype(np.float32)
    nets = []
    for q in range(Q):
        torch.manual_seed(seed + q)
        fl = FeedbackLoopConfig(coupling_matrix_type=CouplingMatrixType.SCALAR, use_zero_coupling=True)
        of = OutputFilterConfig(use_svfs=False, num_hidden_layers=1, num_neurons_per_layer=8, num_fourier_features=3)
        net = DiffDirectionalFDNVarReceiverPos(FS, G, delays, DEV, fl, of, ambi_order=order,
                                               common_decay_times=np.array([[0.05, 0.15]]) * (1.0 + 0.15 * q),
                                               use_colorless_loss=True, analysis_matrix=A)
        nets.append(net.to(DEV).eval())
    z = torch.polar(torch.ones(K), np.pi * torch.arange(K, dtype=torch.float32) / (K - 1)).to(DEV)
    pos = torch.tensor(rng.uniform(0.05, 0.95, size=(6, 3)).astype(np.float32), device=DEV)
    taps = torch.tensor((rng.randn(Q, 33) * np.hanning(35)[1:-1]).astype(np.float32), device=DEV)
    rot = rng.randn(P, Ls, Ls).astype(np.float32) / np.sqrt(Ls)
    hrir = (rng.randn(Ls, 2, 24) * np.exp(-np.arange(24) / 6.0)).astype(np.float32)
    return dict(nets=nets, z=z, pos=pos, taps=taps, rot=rot, hrir=hrir, stim=rng.randn(100).astype(np.float32),
                path=[3, 1, 1, 0, 5, 2, 3, 3, 4])


@pytest.fixture(scope="module", params=[(3, 1, 129, 200), (2, 2, 257, 512)], ids=["Q3-order1-K129", "Q2-order2-K257"])
def bands(request):
    Q, order, K, length = request.param
    b = _nets(Q, order, K, 40 + order)
    b["length"] = length
    from diffgfdn_amd.subband import infer_directional_bands, render_binaural_moving_listener_bands
    b["ambi"] = infer_directional_bands(b["nets"], b["z"], b["pos"], b["taps"], length, directional=False, rows=b["path"])
    b["got"] = render_binaural_moving_listener_bands(b["nets"], b["z"], b["pos"], b["taps"], length, b["hrir"], b["path"],
                                                     b["rot"], b["stim"], update_ms=6.0, alpha=0.5)
    return b


def test_bands_against_float64(bands):
    b = bands
    want = bref.ref_binaural(b["ambi"].cpu().numpy(), b["hrir"], None, b["rot"], b["stim"], FS, 6.0, 0.5)
    got = b["got"]
    assert got.dtype == torch.float32 and tuple(got.shape) == (P * 48, 2) == want.shape
    e = _frac(got.cpu().numpy(), want)
    print(f"[binaural] bands: {e:.3e} of the largest output {np.abs(want).max():.3e}")
    within(e, PARITY, "bands against float64")


def test_bands_chunks_alpha_and_fade(bands):
    from diffgfdn_amd.subband import render_binaural_moving_listener_bands as render
    b = bands
    args = (b["nets"], b["z"], b["pos"], b["taps"], b["length"], b["hrir"], b["path"], b["rot"], b["stim"])
    buf = torch.full((P * 48, 2), SENTINEL, device=DEV)
    assert torch.equal(render(*args, update_ms=6.0, sample_rate=FS, out=buf), b["got"])
    parts = render(*args, update_ms=6.0, chunk=4)                   # (the stock product rounds by the batch's shape)
    within(_frac(parts.cpu().numpy(), b["got"].cpu().numpy().astype(np.float64)), PARITY, "bands in chunks of 4")
    got = render(*args, update_ms=6.0, alpha=0.25, fade_len_ms=3.0)
    want = bref.ref_binaural(b["ambi"].cpu().numpy(), b["hrir"], None, b["rot"], b["stim"], FS, 6.0, 0.25, 3.0)
    within(_frac(got.cpu().numpy(), want), PARITY, "bands alpha 0.25, Fd 24")


def test_directional_bank_render_binaural(bands):
    from diffgfdn_amd.graphstep import DirectionalBank
    b = bands

    class _Step:                                                     # (what render_binaural reads of a bank's steps)
        def __init__(self, net):
            self.tr = type("T", (), {"net": net})()
    bank = DirectionalBank.__new__(DirectionalBank)
    bank.steps = [_Step(n) for n in b["nets"]]
    got = bank.render_binaural(b["z"], b["pos"], b["taps"], b["length"], b["hrir"], b["path"], b["rot"], b["stim"],
                               update_ms=6.0)
    assert torch.equal(got, b["got"])


def test_bands_fallback_beyond_the_limits(bands):
    """more than 32 band signals per channel: the rows are rendered and go through the general function -- forced here on a
    case the kernel path runs too"""
    from diffgfdn_amd import hip_ops as ops
    from diffgfdn_amd import subband
    b = bands
    keep = ops.BINAURAL_MAX_S
    try:
        ops.BINAURAL_MAX_S = 1
        got = subband.render_binaural_moving_listener_bands(b["nets"], b["z"], b["pos"], b["taps"], b["length"], b["hrir"],
                                                            b["path"], b["rot"], b["stim"], update_ms=6.0)
    finally:
        ops.BINAURAL_MAX_S = keep
    within(_frac(got.cpu().numpy(), b["got"].cpu().numpy().astype(np.float64)), PARITY, "fallback against the kernel path")


def test_bands_errors(bands):
    from diffgfdn_amd.subband import render_binaural_moving_listener_bands as render
    b = bands
    Ls = b["rot"].shape[1]
    ok = dict(nets=b["nets"], z_values=b["z"], norm_listener_position=b["pos"], taps=b["taps"], length=b["length"],
              hrir_sh=b["hrir"], path=b["path"], rotations=b["rot"], stimulus=b["stim"], update_ms=6.0)
    nb = 1 << (b["length"] - 1).bit_length()
    for bad in (dict(path=[]), dict(path=None), dict(path=[0, 6]), dict(update_ms=0.1), dict(fade_len_ms=0.0),
                dict(fade_len_ms=6.2), dict(alpha=-0.1), dict(alpha=1.5), dict(update_ms=3.0e7),
                dict(rotations=b["rot"][:-1]), dict(rotations=b["rot"][:, :, :-1]), dict(hrir_sh=b["hrir"][:-1]),
                dict(hrir_sh=b["hrir"][:, :1]), dict(hrir_sh=np.zeros((Ls, 2, nb + 1), dtype=np.float32)),
                dict(stimulus=np.zeros(0, dtype=np.float32)), dict(taps=b["taps"][:-1]), dict(nets=[]), dict(length=8),
                dict(out=torch.zeros(P * 48, device=DEV))):
        with pytest.raises(ValueError):
            render(**dict(ok, **bad))
