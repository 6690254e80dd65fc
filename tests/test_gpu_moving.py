"""A listener moving through a band bank's render in one pass (subband.render_moving_listener_bank, csrc/moving.hip) on the
MI355X.

The render is the reference's ``dynamic_rendering_moving_receiver.filter_overlap_add`` (sound_examples.py:163-226), restated in
float64 in ``tests/moving_listener_ref.py`` and pinned to the reference's own output by ``tests/test_moving_listener_golden.py``.

Bounds (``helpers.rel_err``: the max-norm relative to the largest magnitude of the expected output).
  * the two kernels against float64 on the same float32 inputs: 5e-6, what tests/test_gpu_parity.py asserts of ``rfft_pow2``
    against numpy (they make a few dozen float32 roundings per value, a transform of n = 512 makes as many);
  * ``render_moving_listener`` against the golden cases: 1e-5, what tests/test_gpu_parity.py asserts of ``full_convolve``
    against scipy's fftconvolve -- a segment is one such convolution (forward transforms, a product, an inverse
    transform), the running average has weights that sum to 1 and the cross-fade weights lie in [0, 1];
  * the bank: ``PARITY`` = 1e-4, the bar tests/test_gpu_render.py applies to the render itself against the oracle; what
    follows the render is the linear map above.
Measured on an MI355X: see DESIGN 5.1.5.
"""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import rel_err
from tests.margins import within
from tests.moving_listener_ref import overlap_add, ref_moving_listener
from tests.test_gpu_bank import BANDS, DEV, FS, G, _bank_setup, _build_net, _delays
from tests.test_moving_listener_golden import NUM_CASES, case, fixture

pytestmark = pytest.mark.gpu
KERNEL, CONVOLVE, PARITY = 5e-6, 1e-5, 1e-4
SENTINEL = -12345.0
PATH = [3, 7, 7, 0, 10, 2, 5, 5, 1]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- 1. moving_compose -----------------------------------------------------------------------------------------------
F_K, R_STORE = 257, 11                       # n = 512; two workgroups of 256 bins, the second with one live lane


def _cnoise(rng, shape):
    return ((rng.randn(*shape) + 1j * rng.randn(*shape)) / np.sqrt(2.0)).astype(np.complex64)


def _pitched_c(a: np.ndarray, pitch: int) -> torch.Tensor:
    """a (rows, F) complex64 as the first F columns of a (rows, pitch) device buffer; the padding holds SENTINEL"""
    buf = torch.full((a.shape[0], pitch), SENTINEL, dtype=torch.complex64, device=DEV)
    buf[:, :a.shape[1]] = torch.tensor(a)
    return buf


@functools.lru_cache(maxsize=None)
def _compose_problem(S, alpha):
    rng = np.random.RandomState(100 + S)
    P = len(PATH)
    dh, xh = _cnoise(rng, (R_STORE, F_K)), _cnoise(rng, (P, F_K))
    ch = _cnoise(rng, (max(S, 1), F_K)) / np.sqrt(max(S, 1))
    w = rng.randn(P, max(S, 1)).astype(np.float32)
    r = dh[PATH].astype(np.complex128)
    if S:
        r = r + w.astype(np.float64) @ ch.astype(np.complex128)
    z, e = np.empty((P, F_K), dtype=np.complex128), None
    for k in range(P):
        e = r[k] if k == 0 else alpha * r[k] + (1.0 - alpha) * e
        z[k] = e * xh[k].astype(np.complex128)
    return dh, xh, ch, w, z, e


def _compose(S, alpha, chunk, pitch):
    """moving_compose over the path in chunks of ``chunk`` segments on pitched rows; returns (Z buffer, ema)"""
    from diffgfdn_amd import hip_ops as ops
    dh, xh, ch, w, _, _ = _compose_problem(S, alpha)
    P = len(PATH)
    db, xb, cb = _pitched_c(dh, pitch), _pitched_c(xh, pitch), _pitched_c(ch, pitch)
    zb = torch.full((P, pitch), SENTINEL, dtype=torch.complex64, device=DEV)
    rows, wt = torch.tensor(PATH, device=DEV), torch.tensor(w, device=DEV)
    ema = torch.full((F_K,), SENTINEL, dtype=torch.complex64, device=DEV)
    for k0 in range(0, P, chunk):
        k1 = min(k0 + chunk, P)
        kw = dict(W=wt[k0:k1], Ch=cb[:, :F_K]) if S else {}
        got = ops.moving_compose(db[:, :F_K], xb[k0:k1, :F_K], ema, alpha, k0 == 0, rows=rows[k0:k1], out=zb[k0:k1, :F_K],
                                 **kw)
        assert got.data_ptr() == zb[k0:k1].data_ptr()
    for b in (db, xb, cb):
        assert bool((b[:, F_K:] == SENTINEL).all())
    return zb, ema


@pytest.mark.parametrize("alpha", [0.5, 1.0, 0.25])
@pytest.mark.parametrize("S", [0, 4, 32])
def test_moving_compose_against_float64(S, alpha):
    _, _, _, _, z, e = _compose_problem(S, alpha)
    zb, ema = _compose(S, alpha, len(PATH), F_K + 3)
    assert bool((zb[:, F_K:] == SENTINEL).all()), "nothing is stored behind bin F - 1 of a row"
    ez, ee = rel_err(zb[:, :F_K].cpu().numpy(), z), rel_err(ema.cpu().numpy(), e)
    print(f"[moving_compose] S = {S}, alpha = {alpha}: Z off by {ez:.3e}, the filter state by {ee:.3e}")
    within(ez, KERNEL, f"moving_compose Z S={S} alpha={alpha}")
    within(ee, KERNEL, f"moving_compose ema S={S} alpha={alpha}")
    # chunks of 4 segments (4 + 4 + 1) and another pitch: the bits of the single launch
    z4, ema4 = _compose(S, alpha, 4, F_K + 8)
    assert torch.equal(z4[:, :F_K], zb[:, :F_K]) and torch.equal(ema4, ema)


def test_moving_compose_refuses_bad_arguments():
    from diffgfdn_amd import hip_ops as ops
    d = torch.zeros((R_STORE, F_K), dtype=torch.complex64, device=DEV)
    x = torch.zeros((4, F_K), dtype=torch.complex64, device=DEV)
    ema = torch.zeros((F_K,), dtype=torch.complex64, device=DEV)
    with pytest.raises(RuntimeError, match="rows outside"):
        ops.moving_compose(d, x, ema, 0.5, True, rows=torch.tensor([3, 7, 7, R_STORE], device=DEV))
    assert ops.moving_compose(d, x, ema, 0.5, True, rows=torch.tensor([3, 7, 7, 10], device=DEV)).shape == (4, F_K)
    with pytest.raises(RuntimeError, match="come together"):
        ops.moving_compose(d, x, ema, 0.5, True, W=torch.zeros((4, 2), device=DEV))
    with pytest.raises(RuntimeError, match="at most 32"):
        ops.moving_compose(d, x, ema, 0.5, True, W=torch.zeros((4, 33), device=DEV),
                           Ch=torch.zeros((33, F_K), dtype=torch.complex64, device=DEV))
    with pytest.raises(RuntimeError, match="complex64"):
        ops.moving_compose(d.real.contiguous(), x, ema, 0.5, True)
    with pytest.raises(RuntimeError, match="alpha"):
        ops.moving_compose(d, x, ema, 1.5, True)


# ---- 2. moving_ola ---------------------------------------------------------------------------------------------------
LR = 271


def _ola(s: torch.Tensor, P, h, Fd, chunk):
    from diffgfdn_amd import hip_ops as ops
    out = torch.zeros((P * h,), dtype=torch.float32, device=DEV)
    tails = [torch.full((Fd,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(2)]
    for i, k0 in enumerate(range(0, P, chunk)):
        ops.moving_ola(s[k0:k0 + chunk], k0, P, h, LR, Fd, out, tails[i & 1] if k0 else None, tails[1 - (i & 1)])
    return out


# (P, h, Fd): the golden shape; one segment; a fade over the whole interval; a fade of one sample; h not a multiple of four
# (4-byte accesses whatever the pitch)
@pytest.mark.parametrize("P,h,Fd", [(9, 48, 24), (1, 48, 24), (9, 48, 48), (9, 48, 1), (9, 50, 25)])
def test_moving_ola_against_float64(P, h, Fd):
    rng = np.random.RandomState(P + h + Fd)
    n = 512
    s = rng.randn(P, n).astype(np.float32)
    total, lfull = P * h, h + LR - 1
    want = overlap_add([s[k, :min(lfull, total - k * h)].astype(np.float64) for k in range(P)], h, Fd)
    res = {}
    for pitch in (n, n + 3):                     # 16-byte accesses (where h allows), and rows on 4-byte boundaries
        buf = torch.full((P, pitch), SENTINEL, dtype=torch.float32, device=DEV)
        buf[:, :n] = torch.tensor(s)
        res[pitch] = _ola(buf[:, :n], P, h, Fd, P)
        e = rel_err(res[pitch].cpu().numpy(), want)
        print(f"[moving_ola] {(P, h, Fd)}, pitch {pitch}: off by {e:.3e}")
        within(e, KERNEL, f"moving_ola {(P, h, Fd, pitch)}")
        assert torch.equal(_ola(buf[:, :n], P, h, Fd, P), res[pitch]), "the same call twice: the same bits"
        assert torch.equal(_ola(buf[:, :n], P, h, Fd, 4), res[pitch]), "chunks of 4 segments: the bits of one launch"
        assert bool((buf[:, n:] == SENTINEL).all())
    assert torch.equal(res[n], res[n + 3]), "4-byte accesses give the bits of the 16-byte ones"


def test_moving_ola_refuses_bad_arguments():
    from diffgfdn_amd import hip_ops as ops
    s = torch.zeros((4, 512), dtype=torch.float32, device=DEV)
    out = torch.zeros((9 * 48,), dtype=torch.float32, device=DEV)
    t0, t1 = (torch.zeros((24,), dtype=torch.float32, device=DEV) for _ in range(2))
    with pytest.raises(RuntimeError, match="two buffers"):
        ops.moving_ola(s, 4, 9, 48, LR, 24, out, t0, t0)
    with pytest.raises(RuntimeError, match="two buffers"):
        ops.moving_ola(s, 4, 9, 48, LR, 24, out, None, t1)
    with pytest.raises(RuntimeError, match="Fd <= h"):
        ops.moving_ola(s, 0, 9, 48, LR, 49, out, None, torch.zeros((49,), device=DEV))
    with pytest.raises(RuntimeError, match="at least 318"):
        ops.moving_ola(s[:, :317], 0, 9, 48, LR, 24, out, None, t1)
    with pytest.raises(RuntimeError, match="path of P"):
        ops.moving_ola(s, 6, 9, 48, LR, 24, out, t0, t1)


# ---- 3. any RIR matrix: the golden cases -------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NUM_CASES))
def test_render_moving_listener_equals_the_reference(i):
    from diffgfdn_amd.subband import render_moving_listener
    rirs, path, stim, fs, update_ms, alpha, fade_ms, want = case(fixture(), i)
    got = render_moving_listener(rirs, path, stim, fs, update_ms, alpha, fade_ms)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_cuda
    e = rel_err(got.cpu().numpy(), want)
    print(f"[render_moving_listener] golden case {i}: off by {e:.3e}")
    within(e, CONVOLVE, f"render_moving_listener golden case {i}")
    # device rows, a device path, chunks of 4 segments and a buffer to fill: the same bits
    buf = torch.full(want.shape, SENTINEL, dtype=torch.float32, device=DEV)
    again = render_moving_listener(torch.tensor(rirs, dtype=torch.float32, device=DEV), torch.tensor(path, device=DEV),
                                   torch.tensor(stim), fs, update_ms, alpha, fade_ms, chunk=4, out=buf)
    assert again.data_ptr() == buf.data_ptr() and torch.equal(again, got)


# ---- 4. the bank -----------------------------------------------------------------------------------------------------
NFFT_S, M_S, R_S = 256, 16, 11
UPDATE_MS, FADE_MS = 10.0, 5.0               # h = 80, Fd = 40 at 8 kHz: h + Lr - 1 = 350, n = 512, five segments per sample


def _taps_np(M):
    from scipy.signal import firwin
    return np.stack([firwin(M, [f / np.sqrt(2), f * np.sqrt(2)], pass_zero=False, fs=FS) for f in BANDS])


def _small_data(q, R):
    """tests/test_gpu_bank.py ``_build_data`` at nfft = 256 (RIRs of 256 samples)"""
    from diffgfdn_amd.dataloader import MultiRIRDataset, RoomDataset
    from diffgfdn_amd.synthetic import synthetic_room
    room = synthetic_room(R, G, FS, NFFT_S, seed=10 + q, t60_range=(0.2, 0.5))
    ds = MultiRIRDataset(DEV, RoomDataset(G, FS, room["source_position"], room["receiver_position"],
                                          room["rirs"].copy(), room["common_decay_times"], nfft=NFFT_S, device=DEV))
    return room, ds


def _oracle_render(bank, data, taps_np, nfft):
    """the float64 oracle's forward + numpy irfft + scipy fftconvolve + sum over the bands, as
    tests/test_gpu_render.py::test_infer_bank_matches_infer_bands_and_oracle builds it"""
    from scipy.signal import fftconvolve
    from oracle import gfdn_oracle as orc
    R = len(data[0][1])
    want = np.zeros((R, nfft + taps_np.shape[1] - 1))
    for q in range(len(BANDS)):
        sd = {k: v.detach().cpu() for k, v in bank.band_state_dict(q).items()}
        lin, norm = [], []
        for i in range(64):
            k = f"output_scalars.mlp.model.{i}.weight"
            if k in sd:
                (lin if sd[k].ndim == 2 else norm).append((sd[k], sd[f"output_scalars.mlp.model.{i}.bias"]))
        p = orc.GridModelParams(FS, _delays(q), G, sd["input_gains"], sd["output_gains"], sd["feedback_loop.M"],
                                sd["feedback_loop.alpha"], np.linspace(0.2, 0.5, G)[None, :], lin, norm, 4)
        ds = data[q][1]
        ob = {"z_values": ds.z_values.cpu(), "norm_listener_position": ds.norm_listener_position.cpu(),
              "listener_position": ds.listener_positions.cpu(),
              "target_early_response": ds.early_rir_mag_response.cpu().to(torch.complex128)}
        with torch.no_grad():
            H, _ = orc.grid_model_forward(p, ob)
        h = np.fft.irfft(H.numpy(), axis=-1)
        want += np.stack([fftconvolve(h[r], taps_np[q], mode="full") for r in range(R)])
    return want


@pytest.fixture(scope="module")
def small_bank():
    """3 zero-coupling bands, R = 11, nfft 256, M = 16, perturbed parameters, as ``plain_bank`` of tests/test_gpu_render.py"""
    from diffgfdn_amd.bandbank import BandBank, BandStackedDataset
    nets, data = [], []
    for q in range(len(BANDS)):
        net = _build_net(q)
        with torch.no_grad():
            net.input_gains.mul_(1.0 + 0.1 * q)
        nets.append(net)
        data.append(_small_data(q, R_S))
    bank = BandBank(nets)
    sds = BandStackedDataset([d for _, d in data])
    tp = _taps_np(M_S)
    taps = torch.tensor(tp, dtype=torch.float32, device=DEV)
    stim = np.random.RandomState(7).randn(300)
    return bank, sds, data, taps, tp, stim


def test_bank_against_the_oracle_and_the_general_path(small_bank):
    from diffgfdn_amd.subband import infer_bank, render_moving_listener, render_moving_listener_bank
    bank, sds, data, taps, tp, stim = small_bank
    assert bank.num_bands * bank.num_groups == 9
    got = render_moving_listener_bank(bank, sds, taps, PATH, stim, UPDATE_MS, 0.5, FADE_MS, chunk=4)
    h = int(UPDATE_MS * 1e-3 * FS)
    assert h == 80 and tuple(got.shape) == (len(PATH) * h,) and got.dtype == torch.float32
    # (a) the float64 oracle's render of the same parameters through the restatement
    y64 = _oracle_render(bank, data, tp, NFFT_S)
    want = ref_moving_listener(y64, PATH, stim, FS, UPDATE_MS, 0.5, FADE_MS)
    e_oracle = rel_err(got.cpu().numpy(), want)
    # (b) the general path on infer_bank's rows
    y = infer_bank(bank, sds, taps)
    assert tuple(y.shape) == y64.shape
    general = render_moving_listener(y, PATH, stim, FS, UPDATE_MS, 0.5, FADE_MS)
    e_general = rel_err(got.cpu().numpy(), general.cpu().numpy())
    print(f"[render_moving_listener_bank] vs the oracle's render through the restatement {e_oracle:.3e}, vs "
          f"render_moving_listener(infer_bank) {e_general:.3e} (the render itself vs the oracle: "
          f"{rel_err(y.cpu().numpy(), y64):.3e})")
    within(e_oracle, PARITY, "render_moving_listener_bank vs oracle")
    within(e_general, PARITY, "render_moving_listener_bank vs render_moving_listener(infer_bank)")
    # one chunk, the defaults spelled out, a sequence of taps, a device path and a buffer to fill: the same bits
    buf = torch.empty_like(got)
    again = render_moving_listener_bank(bank, sds, [taps[q] for q in range(len(BANDS))], torch.tensor(PATH, device=DEV),
                                        torch.tensor(stim), UPDATE_MS, 0.5, FADE_MS, sample_rate=FS, chunk=32, out=buf)
    assert again.data_ptr() == buf.data_ptr() and torch.equal(again, got)
    # alpha = 1 (no interpolation) and a fade over the whole interval
    got1 = render_moving_listener_bank(bank, sds, taps, PATH, stim, UPDATE_MS, 1.0, UPDATE_MS)
    e1 = rel_err(got1.cpu().numpy(), ref_moving_listener(y64, PATH, stim, FS, UPDATE_MS, 1.0, UPDATE_MS))
    print(f"[render_moving_listener_bank] alpha = 1, Fd = h vs the oracle: {e1:.3e}")
    within(e1, PARITY, "render_moving_listener_bank alpha=1 Fd=h vs oracle")


def test_bank_direct_render_spectrum_cache(small_bank):
    """(d) built once for the same taps (by identity and by value), rebuilt after an in-place edit of the taps"""
    from diffgfdn_amd.subband import render_moving_listener_bank
    bank, sds, _, taps, _, stim = small_bank
    taps = taps.clone()
    n = 512
    first = render_moving_listener_bank(bank, sds, taps, PATH, stim, UPDATE_MS, 0.5, FADE_MS)
    Dh = sds.direct_render_spectrum(taps, n)
    assert tuple(Dh.shape) == (R_S, n // 2 + 1) and Dh.dtype == torch.complex64
    within(rel_err(Dh.cpu().numpy(), np.fft.rfft(sds.direct_render(taps).cpu().numpy().astype(np.float64), n=n)), KERNEL,
           "direct_render_spectrum vs numpy")
    assert torch.equal(render_moving_listener_bank(bank, sds, taps, PATH, stim, UPDATE_MS, 0.5, FADE_MS), first)
    assert sds.direct_render_spectrum(taps, n) is Dh and sds.direct_render_spectrum(taps.clone(), n) is Dh
    taps.mul_(2.0)                                                                                  # edited in place
    D2 = sds.direct_render_spectrum(taps, n)
    assert D2 is not Dh
    within(rel_err(D2.cpu().numpy(), 2.0 * Dh.cpu().numpy()), KERNEL, "Dh rebuilt from doubled taps")
    doubled = render_moving_listener_bank(bank, sds, taps, PATH, stim, UPDATE_MS, 0.5, FADE_MS)
    within(rel_err(doubled.cpu().numpy(), 2.0 * first.cpu().numpy()), CONVOLVE, "the render of doubled taps")
    assert sds.direct_render_spectrum(taps, 1024) is not D2, "another n is another store"


def test_bank_after_training():
    """(c) three steps of the graphed explicit step change the parameters: the result must move -- stale group spectra would
    not -- and still equal the general path on the new render.  On the bank of tests/test_gpu_bank.py ``_bank_setup``
    (R = 12, nfft 8192): the shape at which the project's tests establish the training step."""
    from diffgfdn_amd.subband import infer_bank, render_moving_listener, render_moving_listener_bank
    nets, data, filt, bank, tr, sds, _ = _bank_setup()
    assert tr._fused is not None, "the explicit step is the one under test"
    taps = torch.tensor(_taps_np(M_S), dtype=torch.float32, device=DEV)
    stim = np.random.RandomState(8).randn(300)
    before = render_moving_listener_bank(bank, sds, taps, PATH, stim, UPDATE_MS, 0.5, FADE_MS, chunk=4).clone()
    sel_steps = [[[0, 3, 5, 7], [1, 2, 8, 11], [4, 6, 9, 10]],
                 [[1, 2, 4, 6], [0, 5, 7, 9], [3, 8, 10, 11]],
                 [[8, 9, 10, 11], [3, 4, 6, 10], [0, 1, 2, 5]]]
    step = tr.graphed(sds, 4, mask_seed=777).capture(sds.global_rows(sel_steps[0]))
    for s in sel_steps:
        step(sds.global_rows(s))
    got = render_moving_listener_bank(bank, sds, taps, PATH, stim, UPDATE_MS, 0.5, FADE_MS, chunk=4)
    want = render_moving_listener(infer_bank(bank, sds, taps), PATH, stim, FS, UPDATE_MS, 0.5, FADE_MS)
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    moved = rel_err(got.cpu().numpy(), before.cpu().numpy())
    print(f"[render_moving_listener_bank] after 3 steps vs render_moving_listener(infer_bank) {e:.3e}; moved by {moved:.3e}")
    within(e, PARITY, "render_moving_listener_bank after training")
    assert moved > 10 * PARITY, "training must change the result"


def test_bank_more_than_32_signals():
    """(e) 9 bands x 4 groups = 36 signals: the rows are rendered with infer_bank and go through the general path; against
    the kernels' direct path, fed by hand with the pre-mixed spectra of the same render in two halves of 18 signals"""
    from diffgfdn_amd import hip_ops as ops
    from diffgfdn_amd.bandbank import BandBank, BandStackedDataset
    from diffgfdn_amd.subband import infer_bank, render_moving_listener, render_moving_listener_bank
    from tests.test_gpu_bank_coupled import _build_data as c_data, _build_net as c_net
    R, Gc, nb = 5, 4, 9
    bank = BandBank([c_net(q, Gc, "zero") for q in range(nb)])
    assert bank.num_bands * bank.num_groups == 36
    sds = BandStackedDataset([c_data(q, Gc, R) for q in range(nb)])
    from scipy.signal import firwin
    centres = np.geomspace(100.0, 2500.0, nb)
    taps = torch.tensor(np.stack([firwin(M_S, [f / np.sqrt(2), f * np.sqrt(2)], pass_zero=False, fs=FS) for f in centres]),
                        dtype=torch.float32, device=DEV)
    path = [4, 0, 0, 3, 1, 2, 2, 4, 1]
    stim = np.random.RandomState(9).randn(300)
    got = render_moving_listener_bank(bank, sds, taps, path, stim, UPDATE_MS, 0.5, FADE_MS, chunk=4)
    y = infer_bank(bank, sds, taps)
    assert torch.equal(got, render_moving_listener(y, path, stim, FS, UPDATE_MS, 0.5, FADE_MS, chunk=4))
    want = ref_moving_listener(y.cpu().numpy(), path, stim, FS, UPDATE_MS, 0.5, FADE_MS)
    e = rel_err(got.cpu().numpy(), want)
    # the direct path: Dh + the first 18 signals composed by the kernel's S > 0 form ... of a render that holds the other 18
    h, Fd, Lr = int(UPDATE_MS * 1e-3 * FS), int(FADE_MS * 1e-3 * FS), y.shape[1]
    n = 1 << (h + Lr - 2).bit_length()
    sel = torch.tensor(path, device=DEV)
    W = bank.render_gains(sds.norm_listener_position, R, sel)
    C = bank.filtered_group_signals(sds.z_values, taps)
    half = ops.render_mix(sds.direct_render(taps), W[:, 18:].contiguous(), C[18:], rows=sel)     # (P, Lr): D + the last 18
    Dh, Ch = ops.rfft_pow2(half, n), ops.rfft_pow2(C[:18], n)
    x = torch.tensor(np.tile(stim.astype(np.float32), 3)[:len(path) * h], device=DEV)
    ema = torch.empty((n // 2 + 1,), dtype=torch.complex64, device=DEV)
    Z = ops.moving_compose(Dh, ops.rfft_pow2(x.view(len(path), h), n), ema, 0.5, True, W=W[:, :18], Ch=Ch)
    direct = torch.zeros_like(got)
    ops.moving_ola(ops.irfft_pow2_fwd(Z, n), 0, len(path), h, Lr, Fd, direct, None, torch.empty((Fd,), device=DEV))
    e_direct = rel_err(got.cpu().numpy(), direct.cpu().numpy())
    print(f"[render_moving_listener_bank] 36 signals: vs the restatement on infer_bank's render {e:.3e}, vs the direct path "
          f"{e_direct:.3e}")
    within(e, PARITY, "render_moving_listener_bank 36 signals vs restatement")
    within(e_direct, PARITY, "render_moving_listener_bank 36 signals vs direct path")


def test_argument_errors(small_bank):
    from diffgfdn_amd.subband import render_moving_listener, render_moving_listener_bank
    bank, sds, _, taps, _, stim = small_bank
    with pytest.raises(ValueError, match="cross-fade"):
        render_moving_listener_bank(bank, sds, taps, PATH, stim, UPDATE_MS, 0.5, 0.0)              # Fd = 0
    with pytest.raises(ValueError, match="cross-fade"):
        render_moving_listener_bank(bank, sds, taps, PATH, stim, UPDATE_MS, 0.5, UPDATE_MS + 1.0)  # Fd = 88 > h = 80
    with pytest.raises(ValueError, match="empty path"):
        render_moving_listener_bank(bank, sds, taps, [], stim)
    with pytest.raises(ValueError, match="rows"):
        render_moving_listener_bank(bank, sds, taps, [0, R_S], stim)
    with pytest.raises(ValueError, match="one row of taps"):
        render_moving_listener_bank(bank, sds, taps[:2], PATH, stim)
    y = torch.zeros((R_S, 271), device=DEV)
    with pytest.raises(ValueError, match="cross-fade"):
        render_moving_listener(y, PATH, stim, FS, UPDATE_MS, 0.5, 0.0)
    with pytest.raises(ValueError, match="empty path"):
        render_moving_listener(y, [], stim, FS)
    with pytest.raises(ValueError, match="alpha"):
        render_moving_listener(y, PATH, stim, FS, alpha=1.5)
