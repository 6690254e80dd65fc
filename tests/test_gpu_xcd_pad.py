"""The odd-length transform's three passes on the grid padded to a multiple of 8 items (csrc/fft.hip, blu_xpad: batches
such as the linear step's 14 pairs of group signals keep every item in one XCD's L2).  Placement must not change a bit:
the padded launches against the same items transformed in batches that take the maps the padded grid did not touch
(8 items: the XCD map of full batches; fewer: the plain map), and against float64 transforms on the CPU."""
import numpy as np
import pytest
import torch

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 65537                     # the only length with the 128 x 512 geometry of the wave-per-tile passes
HALF = (N - 1) // 2
SIGNALS = 27                  # 14 pairs, the last one half empty; [:26] = 13 pairs


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffgfdn_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def data(ops):
    """natural-order spectra, their slot order, time gradients, and the float64 results -- computed once, never written to"""
    gen = torch.Generator().manual_seed(14)
    X = torch.view_as_complex(torch.randn(SIGNALS, HALF + 1, 2, generator=gen, dtype=torch.float64))
    X[:, 0] = X[:, 0].real.to(torch.complex128)
    bins, conj = ops.irfft_slot_order(N, torch.device(DEV))
    bins, conj = bins.cpu(), conj.cpu()
    Xs = torch.empty_like(X)
    Xs[:, 0] = X[:, 0]
    Xs[:, 1:] = torch.where(conj[None, :], X[:, bins].conj(), X[:, bins])
    g = torch.randn(SIGNALS, N, generator=gen, dtype=torch.float64)
    Xg = X.clone().requires_grad_(True)
    x64 = torch.fft.irfft(Xg, n=N)
    x64.backward(g)
    gX = Xg.grad
    gXs = torch.empty_like(gX)
    gXs[:, 0] = gX[:, 0].real.to(torch.complex128)
    gXs[:, 1:] = torch.where(conj[None, :], gX[:, bins].conj(), gX[:, bins])
    return {"X": X.to(torch.complex64).to(DEV), "Xs": Xs.to(torch.complex64).to(DEV), "g": g.float().to(DEV),
            "x64": x64.detach().numpy(), "gXs64": gXs.numpy()}


def _join(t):                   # (B, n) -> (pairs, n, 2), zero partner
    B = t.shape[0]
    npairs = (B + 1) // 2
    pad = torch.zeros((2 * npairs, t.shape[1]), dtype=t.dtype, device=t.device)
    pad[:B] = t
    return pad.reshape(npairs, 2, -1).permute(0, 2, 1).contiguous()


def _split(t2, B):              # (pairs, n, 2) -> (B, n)
    return t2.permute(0, 2, 1).reshape(2 * t2.shape[0], -1)[:B].contiguous()


@pytest.mark.parametrize("B", [27, 26])
def test_pair_forward_on_padded_grid(ops, data, B):
    """14 and 13 pairs (padded to 16) == the same pairs in launches of 8 and of 6 / 5 pairs, bit for bit, the scaled form
    included; == numpy's float64 irfft within the bound of the suite's pair-transform test (2e-6 of the largest sample)"""
    Xs = data["Xs"][:B].contiguous()
    got = ops.irfft_odd_fwd(Xs, N, slots=True, pairs=True)
    want = torch.cat([ops.irfft_odd_fwd(Xs[:16].contiguous(), N, slots=True, pairs=True),
                      ops.irfft_odd_fwd(Xs[16:].contiguous(), N, slots=True, pairs=True)])
    assert got.shape == ((B + 1) // 2, N, 2) and torch.equal(got, want)
    err = rel_err(_split(got, B).cpu().numpy(), data["x64"][:B])
    print("pair forward, %d signals: %.2e of the largest sample from float64" % (B, err))
    assert err < 2e-6
    if B % 2:
        assert float(got[-1, :, 1].abs().max()) < 1e-6 * float(np.abs(data["x64"][:B]).max())
    sc = torch.linspace(0.5, 2.0, B, device=DEV)
    got_s = ops.irfft_odd_fwd(Xs, N, slots=True, pairs=True, oscale=sc)
    want_s = torch.cat([ops.irfft_odd_fwd(Xs[:16].contiguous(), N, slots=True, pairs=True, oscale=sc[:16].contiguous()),
                        ops.irfft_odd_fwd(Xs[16:].contiguous(), N, slots=True, pairs=True, oscale=sc[16:].contiguous())])
    assert torch.equal(got_s, want_s)


@pytest.mark.parametrize("B", [27, 26])
def test_pair_adjoint_on_padded_grid(ops, data, B):
    """the adjoint of the same launches: time order (gather) and the transform's own order with two summed inputs, against
    launches of 8 and 6 / 5 pairs bit for bit; against float64 autograd of torch.fft.irfft within 2e-6 of the largest bin"""
    g2 = _join(data["g"][:B])
    got = ops.irfft_odd_pairs_bwd(g2, N, B)
    want = torch.cat([ops.irfft_odd_pairs_bwd(g2[:8].contiguous(), N, 16),
                      ops.irfft_odd_pairs_bwd(g2[8:].contiguous(), N, B - 16)])
    assert torch.equal(got, want)
    err = rel_err(got.cpu().numpy(), data["gXs64"][:B])
    print("pair adjoint, %d signals: %.2e of the largest bin from float64" % (B, err))
    assert err < 2e-6
    sot = ops.irfft_slot_of_time(N, torch.device(DEV)).long()
    gs = torch.empty_like(g2)
    gs[:, 0] = g2[:, 0]
    gs[:, 1 + sot[1:]] = g2[:, 1:]
    half = 0.5 * gs                                     # (exact halves: their sum on load is gs to the bit)
    assert torch.equal(ops.irfft_odd_pairs_bwd(half, N, B, tslots=True, g2b=half), got)


def test_single_item_transforms_on_padded_grid(ops, data):
    """13 items, one per transform (natural-order spectra, gather and scatter through the permutation): forward and adjoint
    == launches of 8 and 5 items bit for bit; forward == float64 within 2e-6"""
    X = data["X"][:13].contiguous()
    got = ops.irfft_odd_fwd(X, N)
    want = torch.cat([ops.irfft_odd_fwd(X[:8].contiguous(), N), ops.irfft_odd_fwd(X[8:].contiguous(), N)])
    assert torch.equal(got, want)
    assert rel_err(got.cpu().numpy(), data["x64"][:13]) < 2e-6
    g = data["g"][:13].contiguous()
    for slots in (False, True):
        a = ops.irfft_odd_bwd(g, N, HALF + 1, slots=slots)
        b = torch.cat([ops.irfft_odd_bwd(g[:8].contiguous(), N, HALF + 1, slots=slots),
                       ops.irfft_odd_bwd(g[8:].contiguous(), N, HALF + 1, slots=slots)])
        assert torch.equal(a, b)
