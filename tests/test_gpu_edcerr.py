"""EDC matching error of a band bank's render in one pass (subband.edc_error_bank, csrc/edcerr.hip) on the MI355X.

The metric is the reference's ``get_edc_error`` (plot.py:632-661, called from ``plot_edc_error_in_space`` :606-757,
inference.py:594 and spatial_sampling/solver.py:365), restated here in numpy float64 (``ref_*`` below):

  1. L = min(Tx, Ty, int(2 fs))                                                      (plot.py:689-694)
  2. band signals = the first L samples of the causal convolution with the analysis FIRs (a declared input)
  3. E[t] = sum_{u >= t} x[u]^2                      (schroeder_backward_int, normalize=False, discard_last_zeros=False)
  4. dB(v) = max(10 log10(|v| + eps_f32), -200)                                       (utils.py:16-40)
  5. error_db[r][k] = mean_t |dB(E^x) - dB(E^y)|,  rmse[k] = ||error_db[:, k]||_2 / sqrt(R)      (plot.py:656-661)

Bounds.  The kernel against float64 on the same float32 inputs and the end-to-end call against ``infer_bank``'s render
pushed through the restatement are bounded by FOUR TIMES the worst absolute deviation in dB measured on an MI355X over
all cases of the respective test (the factor covers summation orders that change with the compiler's scheduling and the
one-ulp hardware logarithm); the measured figures stand beside the bounds below.
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_bank import BANDS, DEV, FS, NFFT, _bank_setup, _build_data, _build_net

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
M = 129
SENTINEL = -12345.0

# worst |deviation| in dB measured on an MI355X (all shapes, both pitches); the bounds are four times these
KERNEL_ERR_MEASURED, KERNEL_CURVE_MEASURED = 2.092e-5, 8.961e-5         # (both at L = 5; 1.9e-6 and 9.2e-6 for L >= 1027)
KERNEL_ERR_BOUND, KERNEL_CURVE_BOUND = 4 * KERNEL_ERR_MEASURED, 4 * KERNEL_CURVE_MEASURED
# edc_error_bank against infer_bank's render through the float64 restatement (plain, coupled, trained, A != bands, fallback)
BANK_ERR_MEASURED = 1.888e-4               # (the 36-signal bank; A = 2: 1.4e-4, plain / coupled / trained: 7.1e-5 .. 1.1e-4)
BANK_ERR_BOUND = 4 * BANK_ERR_MEASURED


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- the float64 restatement ---------------------------------------------------------------------------------------
def ref_db(v):
    """utils.py:16-40: 10 log10(|v| + eps) with eps of float32, clipped below at -200"""
    return np.maximum(10.0 * np.log10(np.abs(v) + EPS), -200.0)


def ref_edc(x):
    """Schroeder backward integral over the last axis (normalize=False): E[t] = sum_{u >= t} x[u]^2"""
    return np.cumsum((np.asarray(x, dtype=np.float64) ** 2)[..., ::-1], axis=-1)[..., ::-1]


def ref_error(xk_db, yk):
    """plot.py:656-661: mean over time of |dB(E^x) - dB(E^y)|"""
    return np.abs(xk_db - ref_db(ref_edc(yk))).mean(axis=-1)


def ref_band_split(x, at, L):
    from scipy.signal import fftconvolve
    x = np.asarray(x, dtype=np.float64)
    return np.stack([fftconvolve(x, np.asarray(a, dtype=np.float64)[None, :], mode="full", axes=-1)[:, :L] for a in at],
                    axis=1)


def ref_metric(estimated, measured, at, fs):
    L = min(measured.shape[1], estimated.shape[1], int(2 * fs))
    err = ref_error(ref_db(ref_edc(ref_band_split(measured, at, L))), ref_band_split(estimated, at, L))
    return err, np.linalg.norm(err, axis=0) / np.sqrt(err.shape[0])


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------
# (R, A, S, L): the issue's four, then two that reach the launches with 8 and 16 receivers per workgroup (the group grows
# with the number of workgroups: A * ceil(R / 8) >= 512, A * ceil(R / 16) >= 512)
SHAPES = [(1, 1, 0, 5), (3, 2, 1, 1027), (11, 3, 28, 8321), (19, 7, 32, 4100), (600, 7, 8, 1500), (1170, 7, 3, 1100)]


def _pitched(a: np.ndarray, pitch: int) -> torch.Tensor:
    """a (rows, bands, L) as the first L columns of a (rows, bands, pitch) device buffer; the padding holds SENTINEL"""
    buf = torch.full(a.shape[:2] + (pitch,), SENTINEL, dtype=torch.float32, device=DEV)
    buf[:, :, :a.shape[2]] = torch.tensor(a)
    return buf


def _pitch(L, pitch):
    return L + 3 if pitch == "L+3" else (L + 3) // 4 * 4 + 4


@functools.lru_cache(maxsize=None)
def _problem(R, A, S, L):
    """decaying noise: Dk = 0.05 exp(-t / tau) randn, tau = L / 12; Ck with a 10 % longer tau; W ~ randn; the target is the
    float64 dB curve of an independent draw of Dk with 1.3 times the amplitude.  Returns float32 inputs and the float64
    results on exactly those inputs."""
    rng = np.random.RandomState(1000 * R + 100 * A + 10 * S + L % 7)
    t = np.arange(L)
    tau = L / 12.0
    dk = (0.05 * np.exp(-t / tau) * rng.randn(R, A, L)).astype(np.float32)
    ck = (0.05 * np.exp(-t / (1.1 * tau)) * rng.randn(A, S, L)).astype(np.float32)
    w = rng.randn(R, S).astype(np.float32)
    target = 1.3 * 0.05 * np.exp(-t / tau) * rng.randn(R, A, L)
    e_t = ref_edc(target)
    tdb = ref_db(e_t).astype(np.float32)
    y = dk.astype(np.float64) + np.einsum("rs,ast->rat", w.astype(np.float64), ck.astype(np.float64))
    err = np.abs(ref_db(ref_edc(y)) - tdb.astype(np.float64)).mean(axis=-1)
    if L >= 1027:
        # both regimes of the dB stage are exercised and the error is not trivially zero: error_db above 1 dB on average
        # over receivers and bands (a receiver whose random gains happen to match the target's energy lies lower: the
        # smallest entry of these recipes is 0.30 dB, the averages 2.1 .. 12.3 dB)
        assert (tdb > -60.0).mean() >= 0.25 and (e_t < EPS).mean() >= 0.10, (R, A, S, L)
        assert err.mean() > 1.0 and err.min() > 0.1, (R, A, S, L)
    y32 = y.astype(np.float32)
    return dk, ck, w, tdb, ref_db(ref_edc(y32)), err, y32


@pytest.mark.parametrize("pitch", ["L+3", "aligned"])
@pytest.mark.parametrize("R,A,S,L", SHAPES)
def test_edc_err_kernel_against_float64(R, A, S, L, pitch):
    from diffgfdn_amd import hip_ops as ops
    ld = _pitch(L, pitch)
    dk, ck, w, tdb, ycurve, err, y = _problem(R, A, S, L)
    db, tb = _pitched(dk, ld), _pitched(tdb, ld)
    kw = {}
    if S:
        cb = _pitched(ck, ld)
        kw = dict(W=torch.tensor(w, device=DEV), Ck=cb[:, :, :L])
    got = ops.edc_error(db[:, :, :L], tb[:, :, :L], L, **kw)
    assert tuple(got.shape) == (R, A) and got.dtype == torch.float32
    e_err = float(np.abs(got.cpu().numpy().astype(np.float64) - err).max())
    # mode "curve" takes no group signals: the composed signal (float64 compose, rounded once) as Dk, against ITS curve
    ob = torch.full((R, A, ld), SENTINEL, dtype=torch.float32, device=DEV)
    cgot = ops.edc_curve_db(_pitched(y, ld)[:, :, :L], L, out=ob[:, :, :L])
    assert cgot.data_ptr() == ob.data_ptr()
    e_curve = float(np.abs(cgot.cpu().numpy().astype(np.float64) - ycurve).max())
    print(f"[edc_err] {(R, A, S, L, pitch)}: error_db off by {e_err:.3e} dB (values {err.min():.2f} .. {err.max():.2f}), "
          f"curve off by {e_curve:.3e} dB")
    assert bool((ob[:, :, L:] == SENTINEL).all()), "nothing is stored behind sample L - 1 of a row"
    assert bool((db[:, :, L:] == SENTINEL).all()) and bool((tb[:, :, L:] == SENTINEL).all())
    assert e_err <= KERNEL_ERR_BOUND, (R, A, S, L, pitch, e_err)
    assert e_curve <= KERNEL_CURVE_BOUND, (R, A, S, L, pitch, e_curve)


# ---- 2. determinism, rows, S = 0 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", ["L+3", "aligned"])
def test_edc_err_repeats_and_rows(pitch):
    from diffgfdn_amd import hip_ops as ops
    R, A, S, L = SHAPES[2]
    ld = _pitch(L, pitch)
    dk, ck, w, tdb, _, err, y = _problem(R, A, S, L)
    db, tb, cb = _pitched(dk, ld)[:, :, :L], _pitched(tdb, ld)[:, :, :L], _pitched(ck, ld)[:, :, :L]
    wt = torch.tensor(w, device=DEV)
    full = ops.edc_error(db, tb, L, W=wt, Ck=cb)
    assert torch.equal(ops.edc_error(db, tb, L, W=wt, Ck=cb), full), "the same call twice: the same bits"
    sel = [7, 2, 2, 9]
    rows = torch.tensor(sel, device=DEV)
    part = ops.edc_error(db, tb, L, W=wt[rows].contiguous(), Ck=cb, rows=rows)
    assert tuple(part.shape) == (4, A)
    assert torch.equal(part, full[rows]), "a rows subset: the bits of the same rows of the full call"
    c_full = ops.edc_curve_db(db, L)
    assert torch.equal(ops.edc_curve_db(db, L), c_full)
    assert torch.equal(ops.edc_curve_db(db, L, rows=rows), c_full[rows])
    with pytest.raises(RuntimeError, match="rows outside"):
        ops.edc_error(db, tb, L, W=wt[rows].contiguous(), Ck=cb, rows=torch.tensor([7, 2, 2, 11], device=DEV))
    # S = 0 on the pre-mixed band signals (float64 compose rounded once) against the composed call: the bound of test 1
    pre = ops.edc_error(_pitched(y, ld)[:, :, :L], tb, L)
    d = float((pre - full).abs().max())
    print(f"[edc_err] S = 0 on pre-mixed signals vs composed ({pitch}): {d:.3e} dB")
    assert d <= KERNEL_ERR_BOUND
    assert float(np.abs(pre.cpu().numpy() - err).max()) <= KERNEL_ERR_BOUND


def test_edc_err_refuses_bad_arguments():
    from diffgfdn_amd import hip_ops as ops
    d = torch.zeros((3, 2, 16), device=DEV)
    with pytest.raises(RuntimeError, match="come together"):
        ops.edc_error(d, d, 16, W=torch.zeros((3, 1), device=DEV))
    with pytest.raises(RuntimeError, match="at most 32"):
        ops.edc_error(d, d, 16, W=torch.zeros((3, 33), device=DEV), Ck=torch.zeros((2, 33, 16), device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        ops.edc_error(d.double(), d, 16)
    with pytest.raises(RuntimeError, match="float32"):
        ops.edc_curve_db(d, 17)


# ---- 3. - 6. the bank ------------------------------------------------------------------------------------------------
def _firs(centres, scale=1.0):
    from scipy.signal import firwin
    return torch.tensor(np.stack([firwin(M, [f / np.sqrt(2), f * np.sqrt(2)], pass_zero=False, fs=FS) for f in centres])
                        * scale, dtype=torch.float32, device=DEV)


def _noise(R, T, seed, amp=2e-3):
    rng = np.random.RandomState(seed)
    return torch.tensor(amp * np.exp(-np.arange(T) / (T / 10.0)) * rng.randn(R, T), dtype=torch.float32, device=DEV)


def _check_bank(bank, sds, taps, measured, what, **kw):
    """edc_error_bank against infer_bank's render through the float64 restatement; returns (error_db, deviation)"""
    from diffgfdn_amd.subband import edc_error_bank, infer_bank
    at = kw.get("analysis_taps", taps)
    fs = kw.get("sample_rate", FS)
    err, rmse = edc_error_bank(bank, sds, taps, measured, **kw)
    y = infer_bank(bank, sds, taps)
    want, want_rmse = ref_metric(y.cpu().numpy(), measured.cpu().numpy(), at.cpu().numpy(), fs)
    assert tuple(err.shape) == want.shape and tuple(rmse.shape) == (at.shape[0],) and err.dtype == torch.float32
    dev = float(np.abs(err.cpu().numpy() - want).max())
    dev_rmse = float(np.abs(rmse.cpu().numpy() - want_rmse).max())
    print(f"[edc_error_bank] {what}: error_db {want.min():.2f} .. {want.max():.2f} dB, rmse {np.round(want_rmse, 2)}, "
          f"off by {dev:.3e} dB (rmse {dev_rmse:.3e})")
    assert want.mean() > 0.5, "the test's error is of the order of dB"
    assert dev <= BANK_ERR_BOUND and dev_rmse <= BANK_ERR_BOUND, (what, dev, dev_rmse)
    return err, dev


@pytest.fixture(scope="module")
def plain():
    """the 3-band bank of tests/test_gpu_render.py (R = 11, nfft 8192, M = 129); measured = the render of a second,
    differently seeded bank plus decaying noise"""
    from diffgfdn_amd.bandbank import BandBank, BandStackedDataset
    from diffgfdn_amd.subband import infer_bank
    R = 11
    nets, nets2, data = [], [], []
    for q in range(len(BANDS)):
        net = _build_net(q)
        with torch.no_grad():
            net.input_gains.mul_(1.0 + 0.1 * q)
        nets.append(net)
        nets2.append(_build_net(q + 5))
        data.append(_build_data(q, R=R)[1])
    bank, sds, taps = BandBank(nets), BandStackedDataset(data), _firs(BANDS)
    measured = (infer_bank(BandBank(nets2), sds, taps) + _noise(R, NFFT + M - 1, 1)).clone()
    return bank, sds, taps, measured, data, R


def test_edc_error_bank_against_float64(plain):
    from diffgfdn_amd.subband import edc_error_bank
    bank, sds, taps, measured, _, R = plain
    err, _ = _check_bank(bank, sds, taps, measured, "plain bank")
    # numpy measured RIRs and a sequence of taps are the same call; rows: the bits of those rows
    again, _ = edc_error_bank(bank, sds, [taps[q] for q in range(len(BANDS))], measured.cpu().numpy())
    assert torch.equal(again, err)
    sel = [7, 2, 2, 9]
    part, rmse = edc_error_bank(bank, sds, taps, measured, rows=sel)
    assert torch.equal(part, err[torch.tensor(sel, device=DEV)])
    assert torch.allclose(rmse, part.square().mean(0).sqrt(), rtol=1e-6)
    with pytest.raises(ValueError, match="rows"):
        edc_error_bank(bank, sds, taps, measured, rows=[0, R])
    # other analysis bands than the bank's (A = 2 != 3), and L clamped by int(2 fs)
    at = _firs((177.0, 707.0))
    e2, _ = _check_bank(bank, sds, taps, measured, "A = 2, fs = 2000", analysis_taps=at, sample_rate=2000.0)
    assert tuple(e2.shape) == (R, 2)


def test_edc_error_bank_coupled():
    from diffgfdn_amd.bandbank import BandBank, BandStackedDataset
    from diffgfdn_amd.subband import infer_bank
    from tests.test_gpu_bank_coupled import _build_data as c_data, _build_net as c_net
    R, Gc = 11, 3
    gen = torch.Generator(device="cpu").manual_seed(3)
    banks = []
    for off in (0, 5):
        nets = [c_net(q + off, Gc) for q in range(len(BANDS))]
        for net in nets:
            with torch.no_grad():
                a = net.feedback_loop.alpha
                a.copy_((0.4 * torch.randn(a.shape, generator=gen)).to(a.device))
        banks.append(BandBank(nets))
    assert banks[0].coupled
    sds = BandStackedDataset([c_data(q, Gc, R) for q in range(len(BANDS))])
    taps = _firs(BANDS)
    measured = infer_bank(banks[1], sds, taps) + _noise(R, NFFT + M - 1, 2)
    _check_bank(banks[0], sds, taps, measured, "coupled bank")


def test_edc_error_bank_after_training():
    """three steps of the graphed explicit step: the error must have moved, and still match the render's"""
    from diffgfdn_amd.bandbank import BandBank
    from diffgfdn_amd.subband import infer_bank
    nets, data, filt, bank, tr, sds, _ = _bank_setup()
    assert tr._fused is not None
    R = len(sds)
    taps = _firs(BANDS)
    measured = (infer_bank(BandBank([_build_net(q + 5) for q in range(len(BANDS))]), sds, taps)
                + _noise(R, NFFT + M - 1, 3)).clone()
    before, _ = _check_bank(bank, sds, taps, measured, "before training")
    before = before.clone()
    sel_steps = [[[0, 3, 5, 7], [1, 2, 8, 11], [4, 6, 9, 10]],
                 [[1, 2, 4, 6], [0, 5, 7, 9], [3, 8, 10, 11]],
                 [[8, 9, 10, 11], [3, 4, 6, 10], [0, 1, 2, 5]]]
    step = tr.graphed(sds, 4, mask_seed=777).capture(sds.global_rows(sel_steps[0]))
    for s in sel_steps:
        step(sds.global_rows(s))
    after, _ = _check_bank(bank, sds, taps, measured, "after 3 steps")
    moved = float((after - before).abs().max())
    print(f"[edc_error_bank] three steps moved error_db by up to {moved:.3e} dB")
    assert moved > 10 * BANK_ERR_BOUND, "training must change the error"


def test_edc_error_of_rendered_rirs_equals_bank(plain):
    """4. subband.edc_error on infer_bands' output == edc_error_bank"""
    from diffgfdn_amd.subband import edc_error, edc_error_bank
    from tests.test_gpu_render import _infer_bands
    bank, sds, taps, measured, data, R = plain
    y = _infer_bands(bank.nets, data, R, taps)
    err, rmse = edc_error(y, measured, taps, FS)
    want, want_rmse = edc_error_bank(bank, sds, taps, measured)
    d = float((err - want).abs().max())
    print(f"[edc_error] on infer_bands' output vs edc_error_bank: {d:.3e} dB")
    assert d <= BANK_ERR_BOUND and float((rmse - want_rmse).abs().max()) <= BANK_ERR_BOUND
    # (a subset goes through the transforms in other batches than the full call: to the bound, not to the bit)
    sel = [7, 2, 2, 9]
    part = edc_error(y, measured, taps, FS, rows=sel)[0]
    assert float((part - err[torch.tensor(sel, device=DEV)]).abs().max()) <= BANK_ERR_BOUND


def test_edc_error_caches(plain):
    """5. a second call builds nothing; analysis taps edited in place rebuild both constants; other measured RIRs the
    target only"""
    from diffgfdn_amd.subband import edc_error_bank
    bank, sds, taps, measured, _, R = plain
    L = NFFT + M - 1
    at = taps.clone()
    edc_error_bank(bank, sds, taps, measured, analysis_taps=at)
    Dk, Tdb = sds.direct_band_render(taps, at, L), sds.edc_error_target(measured, at, L)
    assert tuple(Dk.shape) == tuple(Tdb.shape) == (R, len(BANDS), L)
    first, _ = edc_error_bank(bank, sds, taps, measured, analysis_taps=at)
    assert sds.direct_band_render(taps, at, L).data_ptr() == Dk.data_ptr()
    assert sds.edc_error_target(measured, at, L).data_ptr() == Tdb.data_ptr()
    assert sds.direct_band_render(taps.clone(), at.clone(), L).data_ptr() == Dk.data_ptr()          # ... by value too
    assert sds.edc_error_target(measured.clone(), at.clone(), L).data_ptr() == Tdb.data_ptr()
    other = measured * 1.5
    second, _ = edc_error_bank(bank, sds, taps, other, analysis_taps=at)
    assert sds.direct_band_render(taps, at, L).data_ptr() == Dk.data_ptr(), "other measured RIRs: Dk stays"
    T2 = sds.edc_error_target(other, at, L)
    assert T2.data_ptr() != Tdb.data_ptr() and not torch.equal(second, first)
    del Tdb
    at.mul_(2.0)                                                                                    # edited in place
    D3, T3 = sds.direct_band_render(taps, at, L), sds.edc_error_target(other, at, L)
    assert D3.data_ptr() != Dk.data_ptr() and T3.data_ptr() != T2.data_ptr()
    assert torch.allclose(D3, 2.0 * Dk, rtol=1e-4, atol=1e-7)


def test_edc_error_bank_more_than_32_signals():
    """6. 9 bands x 4 groups = 36 signals: render_mix per analysis band into a temporary, then the kernel with S = 0"""
    from diffgfdn_amd.bandbank import BandBank, BandStackedDataset
    from diffgfdn_amd.subband import infer_bank
    from tests.test_gpu_bank_coupled import _build_data as c_data, _build_net as c_net
    R, Gc, nb = 5, 4, 9
    centres = np.geomspace(100.0, 2500.0, nb)
    bank = BandBank([c_net(q, Gc, "zero") for q in range(nb)])
    bank2 = BandBank([c_net(q + 11, Gc, "zero") for q in range(nb)])
    assert bank.num_bands * bank.num_groups == 36
    sds = BandStackedDataset([c_data(q, Gc, R) for q in range(nb)])
    taps = _firs(centres)
    measured = infer_bank(bank2, sds, taps) + _noise(R, NFFT + M - 1, 4)
    err, _ = _check_bank(bank, sds, taps, measured, "36 signals")
    from diffgfdn_amd.subband import edc_error_bank
    sel = [4, 0, 0]
    assert torch.equal(edc_error_bank(bank, sds, taps, measured, rows=sel)[0], err[torch.tensor(sel, device=DEV)])
