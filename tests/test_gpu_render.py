"""Full-band render of a band bank in one pass (subband.infer_bank, csrc/render.hip) on the MI355X.

The reference's ``inferencing`` (run_subband_training_treble.py:207-375) renders every receiver of every band
(get_response), filters it with the band's reconstructing FIR and sums the bands per receiver.  Neither transform depends
on the receiver: y[r] = D[r] + sum_s W[r][s] C[s] with D a constant of the dataset, C the bank's bands x G filtered group
signals and W the receiver gains -- one skinny product for all receivers.

  1. the kernel against a float64 D + W @ C, elementwise inside (S + 2) 2^-24 (|D| + |W| @ |C|): the standard bound of
     S + 1 float32 roundings in any order (the kernel makes S: one fused multiply-add per signal);
  2. infer_bank against infer_bands on the same nets and against the CPU oracle's forward + numpy irfft + scipy
     fftconvolve + sum (as tests/test_gpu_inference.py builds it), rel_err < 1e-4, the project's parity bar;
  3. a bank with learnable SCALAR coupling angles; 4. after three steps of the graphed explicit training step;
  5. the cache of the dataset constant, and receiver subsets.
"""
import numpy as np
import pytest
import torch

from tests.helpers import rel_err
from tests.test_gpu_bank import BANDS, DEV, FS, G, NFFT, _bank_setup, _build_data, _build_net, _delays

pytestmark = pytest.mark.gpu
PARITY = 1e-4
M = 129


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- 1. the kernel --------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 5), (3, 9, 1027), (11, 28, 8321), (70, 33, 4100)]
SENTINEL = -12345.0


def _pitched(a: np.ndarray, pitch: int) -> torch.Tensor:
    """a (rows, n) as the first n columns of a (rows, pitch) device buffer; the padding holds SENTINEL"""
    buf = torch.full((a.shape[0], pitch), SENTINEL, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = torch.tensor(a)
    return buf


def _problem(R, S, n, rows_in_d=None):
    rng = np.random.RandomState(1000 * R + 10 * S + n % 7)
    d = rng.randn(rows_in_d or R, n).astype(np.float32)
    w = rng.randn(R, S).astype(np.float32)
    c = rng.randn(S, n).astype(np.float32)
    return d, w, c


def _check(out: np.ndarray, d: np.ndarray, w: np.ndarray, c: np.ndarray, what):
    S = w.shape[1]
    d, w, c = d.astype(np.float64), w.astype(np.float64), c.astype(np.float64)
    ref = d + w @ c
    bound = (S + 2) * 2.0 ** -24 * (np.abs(d) + np.abs(w) @ np.abs(c))
    err = np.abs(out.astype(np.float64) - ref)
    worst = float((err / bound).max())
    print(f"[render_mix] {what}: largest error / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


# pitch n + 3: rows that are not 16-byte aligned (4-byte accesses); "aligned": the next multiple of 4 above it (16-byte accesses)
@pytest.mark.parametrize("pitch", ["n+3", "aligned"])
@pytest.mark.parametrize("R,S,n", SHAPES)
def test_render_mix_against_float64(R, S, n, pitch):
    from diffgfdn_amd import hip_ops as ops
    ld = n + 3 if pitch == "n+3" else (n + 3) // 4 * 4 + 4
    d, w, c = _problem(R, S, n)
    db, cb = _pitched(d, ld), _pitched(c, ld)
    ob = torch.full((R, ld), SENTINEL, dtype=torch.float32, device=DEV)
    got = ops.render_mix(db[:, :n], torch.tensor(w, device=DEV), cb[:, :n], out=ob[:, :n])
    assert got.data_ptr() == ob.data_ptr() and tuple(got.shape) == (R, n)
    torch.cuda.synchronize()
    _check(got.cpu().numpy(), d, w, c, (R, S, n, pitch))
    assert bool((ob[:, n:] == SENTINEL).all()), "nothing is stored behind sample n - 1 of a row"
    # without ``out``: a fresh contiguous result, the same bits
    assert torch.equal(ops.render_mix(db[:, :n], torch.tensor(w, device=DEV), cb[:, :n]), got)


@pytest.mark.parametrize("pitch", ["n+3", "aligned"])
def test_render_mix_in_place(pitch):
    """out = d (S = 33: two launches, the second in place whatever the caller passes): the bits of the out-of-place call"""
    from diffgfdn_amd import hip_ops as ops
    R, S, n = SHAPES[3]
    ld = n + 3 if pitch == "n+3" else (n + 3) // 4 * 4 + 4
    d, w, c = _problem(R, S, n)
    db, cb = _pitched(d, ld), _pitched(c, ld)
    wt = torch.tensor(w, device=DEV)
    want = ops.render_mix(db[:, :n], wt, cb[:, :n])
    got = ops.render_mix(db[:, :n], wt, cb[:, :n], out=db[:, :n])
    assert got.data_ptr() == db.data_ptr()
    _check(got.cpu().numpy(), d, w, c, ("in place", pitch))
    assert torch.equal(got, want)
    assert bool((db[:, n:] == SENTINEL).all())
    with pytest.raises(RuntimeError, match="alias"):
        ops.render_mix(db[:, :n], wt, cb[:, :n], rows=torch.arange(R, device=DEV), out=db[:, :n])


@pytest.mark.parametrize("pitch", ["n+3", "aligned"])
def test_render_mix_rows(pitch):
    """rows = [7, 2, 2, 9] of an 11-row store: inside the bound, and the bits of the same rows of the full call"""
    from diffgfdn_amd import hip_ops as ops
    R, S, n = SHAPES[2]
    ld = n + 3 if pitch == "n+3" else (n + 3) // 4 * 4 + 4
    d, w, c = _problem(R, S, n)
    db, cb = _pitched(d, ld), _pitched(c, ld)
    sel = [7, 2, 2, 9]
    rows = torch.tensor(sel, device=DEV)
    full = ops.render_mix(db[:, :n], torch.tensor(w, device=DEV), cb[:, :n])
    got = ops.render_mix(db[:, :n], torch.tensor(w[sel], device=DEV), cb[:, :n], rows=rows)
    assert tuple(got.shape) == (4, n)
    _check(got.cpu().numpy(), d[sel], w[sel], c, ("rows", pitch))
    assert torch.equal(got, full[rows])
    with pytest.raises(RuntimeError, match="rows outside"):
        ops.render_mix(db[:, :n], torch.tensor(w[sel], device=DEV), cb[:, :n], rows=torch.tensor([7, 2, 2, 11], device=DEV))


# ---- 2. - 5. the bank ----------------------------------------------------------------------------------------------
def _taps():
    from scipy.signal import firwin
    return {f: firwin(M, [f / np.sqrt(2), f * np.sqrt(2)], pass_zero=False, fs=FS) for f in BANDS}


def _taps_tensor(scale=1.0):
    t = _taps()
    return torch.tensor(np.stack([t[f] for f in BANDS]) * scale, dtype=torch.float32, device=DEV)


def _infer_bands(nets, datasets, R, taps):
    """the existing path on the SAME modules: band by band, GridLoader batches of 4 receivers"""
    from diffgfdn_amd.dataloader import GridLoader
    from diffgfdn_amd.subband import infer_bands

    def load_band(f):
        q = BANDS.index(f)
        return nets[q], GridLoader(datasets[q], list(range(R)), batch_size=4, shuffle=False), taps[q]

    return infer_bands(list(BANDS), load_band)


@pytest.fixture(scope="module")
def plain_bank():
    """3 zero-coupling bands, R = 11, perturbed parameters; the band-by-band render of the same nets, computed once"""
    from diffgfdn_amd.bandbank import BandBank, BandStackedDataset
    R = 11
    nets, data = [], []
    for q in range(len(BANDS)):
        net = _build_net(q)
        with torch.no_grad():
            net.input_gains.mul_(1.0 + 0.1 * q)
        nets.append(net)
        data.append(_build_data(q, R=R))
    bank = BandBank(nets)
    sds = BandStackedDataset([d for _, d in data])
    taps = _taps_tensor()
    want = _infer_bands(bank.nets, [d for _, d in data], R, taps).clone()
    return bank, sds, data, taps, want, R


def test_infer_bank_matches_infer_bands_and_oracle(plain_bank):
    from scipy.signal import fftconvolve
    from diffgfdn_amd.subband import infer_bank
    from oracle import gfdn_oracle as orc
    bank, sds, data, taps, want_bands, R = plain_bank
    got = infer_bank(bank, sds, taps)
    assert tuple(got.shape) == (R, NFFT + M - 1) and got.dtype == torch.float32
    e_bands = rel_err(got.cpu().numpy(), want_bands.cpu().numpy())
    # a sequence of per-band taps is the same call
    assert torch.equal(infer_bank(bank, sds, [taps[q] for q in range(len(BANDS))]), got)

    tp = _taps()
    want = np.zeros((R, NFFT + M - 1))
    for q, f in enumerate(BANDS):
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
        want += np.stack([fftconvolve(h[r], tp[f], mode="full") for r in range(R)])
    e_oracle = rel_err(got.cpu().numpy(), want)
    print(f"[infer_bank] vs infer_bands {e_bands:.3e}, vs oracle {e_oracle:.3e}")
    assert e_bands < PARITY
    assert e_oracle < PARITY


def test_infer_bank_coupled():
    """learnable SCALAR coupling angles (the bank's dense-A solve), built as tests/test_gpu_bank_coupled.py builds it"""
    from diffgfdn_amd.bandbank import BandBank, BandStackedDataset
    from diffgfdn_amd.subband import infer_bank
    from tests.test_gpu_bank_coupled import _build_data as c_data, _build_net as c_net
    R, Gc = 11, 3
    nets = [c_net(q, Gc) for q in range(len(BANDS))]
    gen = torch.Generator(device="cpu").manual_seed(3)
    for net in nets:                                      # (angles away from their initial values: a real coupling)
        with torch.no_grad():
            a = net.feedback_loop.alpha
            a.copy_((0.4 * torch.randn(a.shape, generator=gen)).to(a.device))
    data = [c_data(q, Gc, R) for q in range(len(BANDS))]
    bank = BandBank(nets)
    assert bank.coupled
    taps = _taps_tensor()
    got = infer_bank(bank, BandStackedDataset(data), taps)
    want = _infer_bands(bank.nets, data, R, taps)
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    print(f"[infer_bank] coupled bank vs infer_bands {e:.3e}")
    assert e < PARITY


def test_infer_bank_after_training():
    """three steps of the graphed explicit step: stale parameter views, or normalize's scale (it lives in b and c) missing
    from the group signals, would show here"""
    from diffgfdn_amd.subband import infer_bank
    nets, data, filt, bank, tr, sds, _ = _bank_setup()
    assert tr._fused is not None, "the explicit step is the one under test"
    R = len(sds)
    taps = _taps_tensor()
    before = infer_bank(bank, sds, taps).clone()
    sel_steps = [[[0, 3, 5, 7], [1, 2, 8, 11], [4, 6, 9, 10]],
                 [[1, 2, 4, 6], [0, 5, 7, 9], [3, 8, 10, 11]],
                 [[8, 9, 10, 11], [3, 4, 6, 10], [0, 1, 2, 5]]]
    step = tr.graphed(sds, 4, mask_seed=777).capture(sds.global_rows(sel_steps[0]))
    for s in sel_steps:
        step(sds.global_rows(s))
    got = infer_bank(bank, sds, taps)
    want = _infer_bands(bank.nets, [d for _, d in data], R, taps)
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    moved = rel_err(got.cpu().numpy(), before.cpu().numpy())
    print(f"[infer_bank] after 3 steps vs infer_bands {e:.3e}; moved by {moved:.3e}")
    assert e < PARITY
    assert moved > 10 * PARITY, "training must change the render"


def test_direct_render_cache_and_row_subsets(plain_bank):
    from diffgfdn_amd.subband import infer_bank
    bank, sds, data, taps, _, R = plain_bank
    D = sds.direct_render(taps)
    assert tuple(D.shape) == (R, NFFT + M - 1)
    assert sds.direct_render(taps).data_ptr() == D.data_ptr()                  # the same taps: the same storage
    assert sds.direct_render(taps.clone()).data_ptr() == D.data_ptr()          # ... by value too
    other = _taps_tensor(scale=0.5)
    D2 = sds.direct_render(other)
    assert D2.data_ptr() != D.data_ptr()
    assert rel_err(D2.cpu().numpy(), 0.5 * D.cpu().numpy()) < 1e-5
    kept = taps.clone()
    D3 = sds.direct_render(kept)
    kept.mul_(2.0)                                                             # edited in place: rebuilt
    D4 = sds.direct_render(kept)
    assert D4.data_ptr() != D3.data_ptr() and rel_err(D4.cpu().numpy(), 2.0 * D3.cpu().numpy()) < 1e-5

    full = infer_bank(bank, sds, taps)
    sel = [7, 2, 2, 9]
    part = infer_bank(bank, sds, taps, rows=sel)
    assert tuple(part.shape) == (4, NFFT + M - 1)
    assert torch.equal(part, full[torch.tensor(sel, device=DEV)])
    out = torch.empty_like(part)
    assert infer_bank(bank, sds, taps, rows=torch.tensor(sel), out=out).data_ptr() == out.data_ptr()
    assert torch.equal(out, part)
    with pytest.raises(ValueError, match="rows"):
        infer_bank(bank, sds, taps, rows=[0, R])
