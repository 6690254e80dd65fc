"""Spatial render of the directional bands in one pass (subband.infer_directional_bands, csrc/dirrender.hip) on the MI355X.

The reference's ``infer_all_octave_bands_directional_fdn`` (inference.py:676-881) renders every receiver of every band
(get_response), cuts it, optionally converts it to directional RIRs, filters it with the band's reconstructing FIR
(fftconvolve, mode='same') and sums the bands per receiver.  None of the transforms depends on the receiver:
ambi[r][l] = sum_s W[r][s][l] C[s][l], dir[r][j] = sum_l A[j][l] ambi[r][l] -- one fused launch for all receivers.

  1. the kernel against float64, elementwise inside (S + Ls + 2) 2^-24 (|A| @ (|W| . |C|)) -- S roundings of the inner sum
     (one fused multiply-add per signal), Ls of the outer, two to spare; (S + 2) 2^-24 (|W| . |C|) in the ambisonic mode --
     with unaligned and aligned pitches, the padding behind every row untouched;
  2. receiver subsets: the same bits as the full call;
  3. infer_directional_bands on three bands against the by-hand GPU path and against the CPU oracle's forward + numpy irfft
     + scipy fftconvolve(mode='same') + sum, rel_err < 1e-4, the project's parity bar; DirectionalBank.render;
  4. beyond the kernel's limits the stock-operator formulation, inside the same bound;  5. argument errors.
"""
import numpy as np
import pytest
import torch

from tests.helpers import mlp_from_state, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
PARITY = 1e-4
SENTINEL = -12345.0
LENGTH = 700


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- 1. the kernel --------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 1, 5), (3, 3, 4, 5, 1027), (11, 21, 9, 12, 8321), (70, 32, 9, 12, 4100), (5, 6, 16, 32, 2049)]


def _pitched(a: np.ndarray, pitch: int) -> torch.Tensor:
    """a (.., n) as the first n samples of a (.., pitch) device buffer; the padding holds SENTINEL"""
    buf = torch.full(a.shape[:-1] + (pitch,), SENTINEL, dtype=torch.float32, device=DEV)
    buf[..., :a.shape[-1]] = torch.from_numpy(a).to(DEV)
    return buf


_problems = {}


def _problem(shape):
    """inputs, float64 results and bounds of a shape: computed once, shared by the cases, never written"""
    if shape not in _problems:
        R, S, Ls, J, n = shape
        rng = np.random.RandomState(R * 1000 + S)
        W = rng.randn(R, S, Ls).astype(np.float32)
        C = (rng.randn(S * Ls, n) * np.exp(-np.arange(n) / (0.3 * n))).astype(np.float32)
        A = rng.randn(J, Ls).astype(np.float32)
        W64, C64, A64 = W.astype(np.float64), C.astype(np.float64).reshape(S, Ls, n), A.astype(np.float64)
        ambi = np.einsum('rsl,sln->rln', W64, C64)
        mag = np.einsum('rsl,sln->rln', np.abs(W64), np.abs(C64))
        _problems[shape] = dict(W=W, C=C, A=A, ambi=ambi, ambi_bound=(S + 2) * 2.0 ** -24 * mag,
                                dir=np.einsum('jl,rln->rjn', A64, ambi),
                                dir_bound=(S + Ls + 2) * 2.0 ** -24 * np.einsum('jl,rln->rjn', np.abs(A64), mag))
    return _problems[shape]


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("directional", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_dir_render_against_float64(shape, directional, aligned):
    from diffgfdn_amd import hip_ops as ops
    R, S, Ls, J, n = shape
    p = _problem(shape)
    pitch = (n + 3) // 4 * 4 if aligned else n + 3
    rows = J if directional else Ls
    Cd = _pitched(p["C"], pitch)
    buf = torch.full((R, rows, pitch), SENTINEL, dtype=torch.float32, device=DEV)
    Wd = torch.from_numpy(p["W"]).to(DEV)
    Ad = torch.from_numpy(p["A"]).to(DEV) if directional else None
    got = ops.dir_render(Wd, Cd[:, :n], Ls, a=Ad, out=buf[:, :, :n])
    assert got.data_ptr() == buf.data_ptr()
    torch.cuda.synchronize()
    assert bool((buf[:, :, n:] == SENTINEL).all()) and bool((Cd[:, n:] == SENTINEL).all())    # nothing behind sample n - 1
    want, bound = (p["dir"], p["dir_bound"]) if directional else (p["ambi"], p["ambi_bound"])
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"{shape} directional={directional} pitch={pitch}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    fresh = ops.dir_render(Wd, Cd[:, :n], Ls, a=Ad)                   # (without out: the same bits)
    assert tuple(fresh.shape) == (R, rows, n) and torch.equal(fresh, got)


@pytest.mark.parametrize("directional", [True, False])
def test_dir_render_row_subset_same_bits(directional):
    from diffgfdn_amd import hip_ops as ops
    shape = SHAPES[2]
    R, S, Ls, J, n = shape
    p = _problem(shape)
    Wd, Cd = torch.from_numpy(p["W"]).to(DEV), torch.from_numpy(p["C"]).to(DEV)
    Ad = torch.from_numpy(p["A"]).to(DEV) if directional else None
    full = ops.dir_render(Wd, Cd, Ls, a=Ad)
    sel = torch.tensor([7, 2, 2, 9], device=DEV)
    part = ops.dir_render(Wd[sel], Cd, Ls, a=Ad)
    assert torch.equal(part, full[sel])


def test_dir_render_argument_checks():
    from diffgfdn_amd import hip_ops as ops
    W, C, A = (torch.zeros(3, 2, 4, device=DEV), torch.zeros(8, 40, device=DEV), torch.zeros(5, 4, device=DEV))
    with pytest.raises(RuntimeError):
        ops.dir_render(W, C[:7], 4)                                    # rows of c: no multiple of Ls
    with pytest.raises(RuntimeError):
        ops.dir_render(W, C, 4, a=torch.zeros(5, 3, device=DEV))
    with pytest.raises(RuntimeError):
        ops.dir_render(W, C, 4, a=A, out=torch.zeros(3, 4, 40, device=DEV))           # out for the other mode
    with pytest.raises(RuntimeError):
        ops.dir_render(W, C.double(), 4)
    big = torch.zeros(3 * 4 * 40 + 8 * 40, device=DEV)
    with pytest.raises(RuntimeError):                                  # out overlaps c
        ops.dir_render(W, big[:320].view(8, 40), 4, out=big[160:160 + 480].view(3, 4, 40))
    with pytest.raises(RuntimeError):                                  # beyond the limits: no quiet fall-back here
        ops.dir_render(torch.zeros(2, 33, 4, device=DEV), torch.zeros(33 * 4, 16, device=DEV), 4)


# ---- 3. the API -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bands():
    from tests.test_gpu_parity import _directional_bands
    trs, batches = _directional_bands(False, 3)
    rng = np.random.RandomState(19)
    taps = {M: torch.tensor((rng.randn(3, M) * np.hanning(M + 2)[1:-1]).astype(np.float32), device=DEV) for M in (129, 64)}
    return trs, batches, taps


def _by_hand(trs, batches, taps, directional):
    """band by band: get_response -> cut -> ops.sh_to_directional -> same-mode convolution -> sum"""
    from diffgfdn_amd import hip_ops as ops
    from diffgfdn_amd.subband import full_convolve
    from diffgfdn_amd.trainer import get_response
    total, M = 0, taps.shape[1]
    for q, (tr, b) in enumerate(zip(trs, batches)):
        h = get_response(b, tr.net)[-1][..., :LENGTH].contiguous()                    # (R, Ls, L)
        if directional:
            B, Ls, L = h.shape
            hc = torch.view_as_complex(h.view(B, Ls, L // 2, 2))
            h = torch.view_as_real(ops.sh_to_directional(tr.net.sh_output_scalars.analysis_matrix, hc)).reshape(B, -1, L)
        y = full_convolve(h.reshape(-1, LENGTH).contiguous(), taps[q])[:, (M - 1) // 2:(M - 1) // 2 + LENGTH]
        total = total + y.reshape(h.shape)
    return total


def _cpu_chain(trs, batches, taps, directional):
    """oracle.directional_forward + numpy irfft + scipy fftconvolve(mode='same') + sum, float64"""
    from scipy.signal import fftconvolve
    from oracle import gfdn_oracle as orc
    from tests.helpers import load
    delays = torch.tensor(load("f6_directional.npz")["delays"], dtype=torch.float32)  # (the size _directional_bands builds)
    total = 0
    for q, (tr, b) in enumerate(zip(trs, batches)):
        net = tr.net
        sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        G, n = net.num_groups, net.num_delay_lines_per_group
        z = b["z_values"].cpu()
        Afb = orc.coupled_feedback_matrix(sd["feedback_loop.M"], sd["feedback_loop.alpha"])
        P = orc.feedback_loop_forward(z, delays, sd["delay_filters"], Afb)
        lin, norm = mlp_from_state({"sd_" + k: v.numpy() for k, v in sd.items()}, root="sh_output_scalars.mlp.model.")
        enc = orc.sinusoidal_encoding(b["norm_listener_position"].cpu(), 3)
        w = orc.normalise_sh_weights(orc.mlp_forward(enc, lin, norm).reshape(-1, G, n))
        H = orc.directional_forward(z, sd["input_gains"], sd["output_gains"], w, P, G, n).detach().numpy()
        h = np.fft.irfft(H.astype(np.complex128), n=2 * (H.shape[-1] - 1), axis=-1)[..., :LENGTH]
        if directional:
            h = np.einsum('jl,blk->bjk', net.sh_output_scalars.analysis_matrix.cpu().numpy().astype(np.float64), h)
        total = total + np.stack([fftconvolve(h[r], taps[q].cpu().numpy().astype(np.float64)[None, :], mode='same')
                                  for r in range(h.shape[0])])
    return total


@pytest.mark.parametrize("M", [129, 64])
@pytest.mark.parametrize("directional", [True, False])
def test_infer_directional_bands(bands, directional, M):
    from diffgfdn_amd.subband import infer_directional_bands
    trs, batches, taps = bands
    nets = [tr.net for tr in trs]
    b0 = batches[0]
    got = infer_directional_bands(nets, b0["z_values"], b0["norm_listener_position"], taps[M], LENGTH, directional=directional)
    A = nets[0].sh_output_scalars.analysis_matrix
    R = b0["norm_listener_position"].shape[0]
    assert tuple(got.shape) == (R, A.shape[0] if directional else A.shape[1], LENGTH) and got.dtype == torch.float32
    hand = _by_hand(trs, batches, taps[M], directional)
    cpu = _cpu_chain(trs, batches, taps[M], directional)
    e_hand, e_cpu = rel_err(got.cpu().numpy(), hand.cpu().numpy()), rel_err(got.cpu().numpy(), cpu)
    print(f"M = {M}, directional = {directional}: rel_err by hand {e_hand:.3e}, CPU float64 {e_cpu:.3e}")
    assert e_hand < PARITY and e_cpu < PARITY
    # receiver subsets and a buffer to fill: the same bits
    sub = infer_directional_bands(nets, b0["z_values"], b0["norm_listener_position"], taps[M], LENGTH,
                                  directional=directional, rows=[2, 0, 0])
    assert torch.equal(sub, got[[2, 0, 0]])
    buf = torch.full((R, got.shape[1], LENGTH + 3), SENTINEL, device=DEV)
    infer_directional_bands(nets, b0["z_values"], b0["norm_listener_position"], taps[M], LENGTH, directional=directional,
                            out=buf[:, :, :LENGTH])
    assert torch.equal(buf[:, :, :LENGTH], got) and bool((buf[:, :, LENGTH:] == SENTINEL).all())


def test_directional_bank_render(bands):
    from diffgfdn_amd.graphstep import DirectionalBank
    from diffgfdn_amd.subband import infer_directional_bands
    trs, batches, taps = bands
    b0 = batches[0]
    want = infer_directional_bands([tr.net for tr in trs], b0["z_values"], b0["norm_listener_position"], taps[64], LENGTH)
    bank = DirectionalBank(trs, batches, lanes=2)
    try:
        got = bank.render(b0["z_values"], b0["norm_listener_position"], taps[64], LENGTH)
    finally:
        bank.close()
    assert torch.equal(got, want)


def test_length_is_clamped(bands):
    from diffgfdn_amd.subband import infer_directional_bands
    trs, batches, taps = bands
    b0 = batches[0]
    nfft = 2 * (b0["z_values"].shape[-1] - 1)
    got = infer_directional_bands([tr.net for tr in trs], b0["z_values"], b0["norm_listener_position"], taps[64], 10 * nfft)
    assert got.shape[-1] == nfft


# ---- 4. beyond the kernel's limits ----------------------------------------------------------------------------------
@pytest.mark.parametrize("directional", [True, False])
def test_fallback_meets_the_bound(directional):
    from diffgfdn_amd.subband import directional_mix
    shape = (4, 33, 4, 5, 1000)
    R, S, Ls, J, n = shape
    p = _problem(shape)
    got = directional_mix(torch.from_numpy(p["W"]).to(DEV), torch.from_numpy(p["C"]).to(DEV), Ls,
                          torch.from_numpy(p["A"]).to(DEV) if directional else None)
    want, bound = (p["dir"], p["dir_bound"]) if directional else (p["ambi"], p["ambi_bound"])
    assert tuple(got.shape) == want.shape
    assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= bound).all()


# ---- 5. argument errors ---------------------------------------------------------------------------------------------
def test_argument_errors(bands):
    from diffgfdn_amd.subband import infer_directional_bands
    trs, batches, taps = bands
    nets = [tr.net for tr in trs]
    z, pos = batches[0]["z_values"], batches[0]["norm_listener_position"]
    with pytest.raises(ValueError):
        infer_directional_bands(nets, z, pos, taps[64][:2], LENGTH)                   # taps rows != bands
    with pytest.raises(ValueError):
        infer_directional_bands(nets, z, pos, taps[64], LENGTH, rows=[])
    with pytest.raises(ValueError):
        infer_directional_bands(nets, z, pos, taps[64], LENGTH, rows=[pos.shape[0]])  # a row outside the range
    sh = nets[1].sh_output_scalars
    keep = sh.analysis_matrix
    try:
        sh.analysis_matrix = keep + 0.5
        with pytest.raises(ValueError):
            infer_directional_bands(nets, z, pos, taps[64], LENGTH)                   # mismatched analysis matrices
    finally:
        sh.analysis_matrix = keep
