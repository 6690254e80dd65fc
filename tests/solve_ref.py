"""A float64 reference of the per-bin resolvent solve for the kernel tests (csrc/solve.hip): plain torch in complex128,
no project code in the arithmetic.

    T_k = diag(z_k^m * ig [* igz_k]) - A        (A^T when transposed;  A_k = BM o kron(Phi_k, 1) with filter coupling)
    Y_k = T_k^-1 b

``solve_ref`` solves block by block (the blocks of a bin do not interact: (K, nblk) systems of nper lines, so that a
bank of 65 blocks costs 65 small solves per bin, not one of 260 lines); ``solve_phi_ref`` solves the dense system.  Both
return the gradients of  L = sum Re(Y) Re(gY) + Im(Y) Im(gY)  from autograd -- gY is the cotangent dL/dRe Y + i dL/dIm Y
the kernels are handed -- and the 2-norm condition number of every bin's whole system.

Inputs are taken as given: a test that wants to leave the rounding of the inputs out of the comparison rounds them to
the kernel's formats first (``f32`` / ``c64``) and hands the same values to both sides."""
import numpy as np
import torch

C128 = torch.complex128


def f32(t):
    """the values a float32 kernel argument holds, in float64"""
    return t.to(torch.float32).to(torch.float64)


def c64(t):
    return t.to(torch.complex64).to(C128)


def grid(K):
    """K points on the upper unit half circle, both ends included (z = 1 alone for K = 1)"""
    return torch.exp(1j * np.pi * torch.arange(K, dtype=torch.float64) / max(K - 1, 1)).to(C128)


def _loss(Y, gY):
    return (Y.real * gY.real + Y.imag * gY.imag).sum()


def _cond_bins(T):
    """T (K, nblk, n, n): 2-norm condition number of the block-diagonal system of every bin"""
    if T.shape[-1] == 1:
        s = T.abs().reshape(T.shape[0], -1)
        return s.max(1).values / s.min(1).values
    s = torch.linalg.svdvals(T)
    return s[..., 0].max(1).values / s[..., -1].min(1).values


def solve_ref(z, delays, ig, A, b, transpose=False, igz=None, gY=None):
    """z (K) complex128, delays / ig / b (N) float64, A (nblk, n, n) float64, igz (K, N) complex128 or None,
    gY (K, N) complex128 or None  ->  dict(Y (K, N), cond (K)[, gA, gb, gig])"""
    nblk, n, _ = A.shape
    K, N = z.numel(), nblk * n
    A, b, ig = (t.detach().clone().requires_grad_(gY is not None) for t in (A, b, ig))
    d = z[:, None] ** delays[None, :] * ig[None, :]
    if igz is not None:
        d = d * igz
    Ab = (A.transpose(1, 2) if transpose else A).to(C128)
    T = torch.diag_embed(d.reshape(K, nblk, n)) - Ab[None]
    rhs = b.to(C128).reshape(1, nblk, n, 1).expand(K, nblk, n, 1)
    Y = torch.linalg.solve(T, rhs).reshape(K, N)
    out = {"Y": Y.detach(), "cond": _cond_bins(T.detach())}
    if gY is not None:
        _loss(Y, gY).backward()
        out.update(gA=A.grad, gb=b.grad, gig=ig.grad)
    return out


def solve_dense_ref(z, delays, ig, A, b, transpose=False, igz=None):
    """the same Y and condition numbers from ONE dense N x N system per bin (the check of the block-wise form)"""
    Af = torch.block_diag(*A).to(C128)
    d = z[:, None] ** delays[None, :] * ig[None, :]
    if igz is not None:
        d = d * igz
    T = torch.diag_embed(d) - (Af.T if transpose else Af)[None]
    Y = torch.linalg.solve(T, b.to(C128)[None, :, None].expand(z.numel(), -1, 1)).squeeze(-1)
    return {"Y": Y, "cond": torch.linalg.cond(T)}


def solve_phi_ref(z, delays, ig, BM, Phi, nper, b, igz=None, gY=None):
    """filter coupling: BM (N, N) float64, Phi (K, G, G) complex128  ->  dict(Y, cond[, gBM, gPhi, gb, gig]);
    gPhi (K, G, G) = dL/dRe Phi + i dL/dIm Phi"""
    K, N = z.numel(), BM.shape[0]
    BM, Phi, b, ig = (t.detach().clone().requires_grad_(gY is not None) for t in (BM, Phi, b, ig))
    d = z[:, None] ** delays[None, :] * ig[None, :]
    if igz is not None:
        d = d * igz
    Ak = BM.to(C128)[None] * Phi.repeat_interleave(nper, 1).repeat_interleave(nper, 2)
    T = torch.diag_embed(d) - Ak
    Y = torch.linalg.solve(T, b.to(C128)[None, :, None].expand(K, N, 1)).squeeze(-1)
    out = {"Y": Y.detach(), "cond": torch.linalg.cond(T.detach())}
    if gY is not None:
        _loss(Y, gY).backward()
        out.update(gBM=BM.grad, gPhi=Phi.grad, gb=b.grad, gig=ig.grad)
    return out


def per_bin_err(Y, ref):
    """max over k of  (max_n |Y[k,n] - Yref[k,n]| / max_n |Yref[k,n]|) / cond_k :  the error of every bin on that bin's
    own scale, in units of its condition number -- a wrong bin away from a resonance peak cannot hide behind the peak"""
    Y = Y.detach().cpu().to(C128)
    Yr = ref["Y"]
    e = (Y - Yr).abs().max(1).values / Yr.abs().max(1).values
    return float((e / ref["cond"]).max())
