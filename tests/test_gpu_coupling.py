"""Coupled feedback matrices of all bands in one launch (csrc/coupling.hip: gfdn_coupled_feedback_fwd / _bwd) on the MI355X.

A = block_M o kron(Phi(alpha), 1) and its adjoint against the float64 restatement of the reference under autograd
(oracle.gfdn_oracle.coupled_feedback_matrix), for three bands with different parameters: band 0 has an angle beyond +pi,
band 1 one beyond -pi (clamped: the gradient there is exactly zero), band 2 has alpha = 0 (Phi = I: the off-diagonal blocks
are exactly zero).

Bounds.  A and Phi: 1e-5 of the largest entry (the bound of A in test_f1_feedback_loop).  Gradients (dL/dM through the
rotations' adjoint, dL/dalpha): TWICE what the float32 torch build of the same matrix (FeedbackLoop._real_feedback_matrix under
autograd on the GPU, same inputs, same random dL/dA) leaves against float64, measured in the test -- a different summation
order of the same float32 data may cost a factor of two and nothing more.  Measured on an MI355X, error / largest entry:

    (G, n)    dL/dM kernel   dL/dM torch    dL/dalpha kernel   dL/dalpha torch
    (1, 4)    4.1e-08        6.4e-08        --                 --
    (2, 1)    0 (exactly)    0 (exactly)    6.0e-08            6.0e-08
    (2, 4)    6.9e-08        8.8e-08        5.2e-08            2.7e-08
    (3, 4)    8.3e-08        1.2e-07        4.2e-08            9.9e-08
    (4, 4)    5.3e-08        8.4e-08        5.3e-08            1.1e-07
    (4, 8)    5.6e-08        1.2e-07        6.3e-08            1.3e-07

(G = 2 has one angle per band, two of them clamped by the inputs this file fixes: its dL/dalpha figure is the rounding of ONE
float32 number, half a unit in the last place at most = 6e-8.)
"""
import functools

import numpy as np
import pytest
import torch

from tests.margins import within

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 4), (2, 1), (2, 4), (3, 4), (4, 4), (4, 8)]
NB = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _err(a, ref):
    ref = ref.to(torch.float64)
    scale = float(ref.abs().max())
    return float((a.detach().cpu().to(torch.float64) - ref).abs().max()) / (scale if scale > 0 else 1.0)


@functools.lru_cache(maxsize=None)
def _case(G, n):
    """Inputs (float32, CPU) and the float64 reference of one shape: built once, shared, never written to."""
    from oracle import gfdn_oracle as orc
    g = torch.Generator().manual_seed(1000 * G + n)
    P = G * (G - 1) // 2
    N = G * n
    M = ((2 * torch.rand(NB, G, n, n, generator=g) - 1) / np.sqrt(n)).to(torch.float32)
    alpha = (2 * torch.rand(NB, P, generator=g) - 1).to(torch.float32)
    if P:
        alpha[0, 0] = np.pi + 0.3
        alpha[1, P - 1] = -np.pi - 0.5
        alpha[2] = 0.0
    gA = torch.randn(NB, N, N, generator=g).to(torch.float32)
    A, Phi, gM, galpha = [], [], [], []
    for q in range(NB):
        M64 = M[q].to(torch.float64).requires_grad_(True)
        a64 = alpha[q].to(torch.float64).requires_grad_(True)
        Aq = orc.coupled_feedback_matrix(M64, a64)
        (Aq * gA[q].to(torch.float64)).sum().backward()
        A.append(Aq.detach())
        phi = orc.nd_unitary(a64.detach().clamp(min=-np.pi, max=np.pi), G)
        Phi.append(torch.ones(1, 1, dtype=torch.float64) if G == 1 else phi)
        gM.append(M64.grad)
        galpha.append(a64.grad if P else torch.zeros(0, dtype=torch.float64))
    return M, alpha, gA, torch.stack(A), torch.stack(Phi), torch.stack(gM), torch.stack(galpha)


def _kernel_path(M, alpha, gA, G, n, nbands):
    """(A, Phi, dL/dM, dL/dalpha) through OrthoParam and CoupledFeedback for ``nbands`` bands in one launch each way."""
    from diffgfdn_amd.functional import CoupledFeedback, OrthoParam
    Md = M.to(DEV).reshape(nbands * G, n, n).clone().requires_grad_(True)
    ad = alpha.to(DEV).clone().requires_grad_(True)
    Q, _ = OrthoParam.apply(Md)
    A, Phi = CoupledFeedback.apply(Q, ad, G, n, nbands)
    assert not Phi.requires_grad
    A.backward(gA.to(DEV))
    ga = ad.grad if ad.grad is not None else torch.zeros_like(ad)
    return A.detach(), Phi, Md.grad.reshape(nbands, G, n, n), ga


def _torch_path(M, alpha, gA, G, n):
    """dL/dM, dL/dalpha of the float32 torch build of the same matrices (one FeedbackLoop per band)."""
    from diffgfdn_amd.config import CouplingMatrixType
    from diffgfdn_amd.feedback_loop import FeedbackLoop
    gM, galpha = [], []
    for q in range(M.shape[0]):
        fl = FeedbackLoop(8000.0, G, n, torch.arange(100, 100 + G * n), False, CouplingMatrixType.SCALAR,
                          use_zero_coupling=False, gains=torch.ones(G * n)).to(DEV)
        with torch.no_grad():
            fl.M.copy_(M[q])
            fl.alpha.copy_(alpha[q])
        fl.new_forward()
        fl._real_feedback_matrix().backward(gA[q].to(DEV))
        gM.append(fl.M.grad.detach().cpu())
        galpha.append(fl.alpha.grad.detach().cpu() if fl.alpha.grad is not None else torch.zeros(alpha.shape[1]))
    return torch.stack(gM), torch.stack(galpha)


@pytest.mark.parametrize("G,n", SHAPES)
def test_coupled_feedback_against_float64(G, n):
    M, alpha, gA, A64, Phi64, gM64, ga64 = _case(G, n)
    P = G * (G - 1) // 2
    A, Phi, gM, ga = _kernel_path(M, alpha, gA, G, n, NB)
    assert A.shape == (NB, G * n, G * n) and Phi.shape == (NB, G, G) and ga.shape == (NB, P)
    within(_err(A, A64), 1e-5, ("coupling A", G, n))
    within(_err(Phi, Phi64), 1e-5, ("coupling Phi", G, n))
    if G > 1:
        # alpha = 0: Phi = I, the off-diagonal blocks are exactly zero
        blocks = A[2].reshape(G, n, G, n)
        for i in range(G):
            for j in range(G):
                if i != j:
                    assert torch.equal(blocks[i, :, j, :], torch.zeros(n, n, device=DEV)), (i, j)
        assert torch.equal(Phi[2], torch.eye(G, device=DEV))
        # clamped angles: no gradient, exactly
        assert float(ga[0, 0]) == 0.0 and float(ga[1, P - 1]) == 0.0
        assert float(ga64[0, 0]) == 0.0 and float(ga64[1, P - 1]) == 0.0
    # gradients: twice what the float32 torch build of the same matrices leaves against float64
    tM, ta = _torch_path(M, alpha, gA, G, n)
    eM_t, eM_k = _err(tM, gM64), _err(gM, gM64)
    print(f"[coupling] (G, n) = ({G}, {n}): dL/dM kernel {eM_k:.3e} torch {eM_t:.3e}", end="")
    if P:
        ea_t, ea_k = _err(ta, ga64), _err(ga, ga64)
        print(f"  dL/dalpha kernel {ea_k:.3e} torch {ea_t:.3e}")
        within(ea_k, 2 * ea_t, ("coupling dL/dalpha", G, n))
    else:
        print()
    if n == 1:
        assert not gM.any() and not gM64.any()          # (a 1 x 1 block has no skew part: Q = 1 whatever M is)
    else:
        within(eM_k, 2 * eM_t, ("coupling dL/dM", G, n))


@pytest.mark.parametrize("G,n", SHAPES)
def test_banded_launch_equals_per_band_launches_and_is_deterministic(G, n):
    from diffgfdn_amd import hip_ops as ops
    M, alpha, gA, *_ = _case(G, n)
    Q, _ = ops.ortho_fwd(M.to(DEV).reshape(NB * G, n, n))
    ad, gd = alpha.to(DEV), gA.to(DEV)
    A, Phi = ops.coupled_feedback_fwd(Q, ad, G, n, NB)
    gQ, ga = ops.coupled_feedback_bwd(Q, ad, G, n, NB, gd)
    A2, Phi2 = ops.coupled_feedback_fwd(Q, ad, G, n, NB)
    gQ2, ga2 = ops.coupled_feedback_bwd(Q, ad, G, n, NB, gd)
    assert torch.equal(A, A2) and torch.equal(Phi, Phi2) and torch.equal(gQ, gQ2) and torch.equal(ga, ga2)
    for q in range(NB):
        Qq = Q[q * G:(q + 1) * G].contiguous()
        Aq, Phiq = ops.coupled_feedback_fwd(Qq, ad[q:q + 1], G, n, 1)
        gQq, gaq = ops.coupled_feedback_bwd(Qq, ad[q:q + 1], G, n, 1, gd[q:q + 1].contiguous())
        assert torch.equal(A[q], Aq[0]) and torch.equal(Phi[q], Phiq[0]), q
        assert torch.equal(gQ[q * G:(q + 1) * G], gQq) and torch.equal(ga[q], gaq[0]), q


def test_argument_guards():
    from diffgfdn_amd import hip_ops as ops
    G, n = 4, 9                                               # G nper = 36 > GFDN_MAX_BLOCK
    Q = torch.zeros(G, n, n, device=DEV)
    alpha = torch.zeros(1, 6, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported size"):
        ops.coupled_feedback_fwd(Q, alpha, G, n, 1)
    with pytest.raises(RuntimeError, match="unsupported size"):
        ops.coupled_feedback_bwd(Q, alpha, G, n, 1, torch.zeros(1, 36, 36, device=DEV))
    with pytest.raises(RuntimeError, match="unsupported size"):      # more groups than GFDN_MAX_GROUPS
        ops.coupled_feedback_fwd(torch.zeros(9, 2, 2, device=DEV), torch.zeros(1, 36, device=DEV), 9, 2, 1)
    with pytest.raises(RuntimeError):                                # shapes that do not match the sizes
        ops.coupled_feedback_fwd(torch.zeros(3, 4, 4, device=DEV), torch.zeros(1, 6, device=DEV), 4, 4, 1)
    lib = ops._lib.load()
    assert lib.gfdn_coupled_feedback_fwd(None, None, 1, 2, 2, None, None, None) == -1
    assert lib.gfdn_coupled_feedback_bwd(None, None, 0, 2, 2, None, None, None, None) == -1
