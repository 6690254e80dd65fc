"""CPU checks around the resolvent solve: the block-wise float64 reference of tests/solve_ref.py against one dense
N x N solve per bin, and the dispatch rule of the launchers (a host-side query: no GPU) over the parameter lists of
tests/test_gpu_solve_paths.py."""
import os
import subprocess

import pytest
import torch

from tests import solve_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip_ops():
    from diffgfdn_amd import _lib, hip_ops
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "diffgfdn_amd", "csrc"), "-j4"])
    _lib.load()
    return hip_ops


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("absorb", [False, True])
def test_blockwise_reference_equals_dense_solve(transpose, absorb):
    from tests.test_gpu_solve_paths import _absorption, _cotangent, float32_inputs
    nblk, nper, K = 3, 5, 9
    N = nblk * nper
    A, delays, ig, b = float32_inputs(nblk, nper)
    z = ref.grid(K) * 1.0003
    igz = _absorption(K, N, 5) if absorb else None
    gY = _cotangent(K, N, 5)
    r = ref.solve_ref(z, delays, ig, A, b, transpose, igz, gY)
    d = ref.solve_dense_ref(z, delays, ig, A, b, transpose, igz)
    assert float((r["Y"] - d["Y"]).abs().max() / d["Y"].abs().max()) < 1e-13
    assert float((r["cond"] / d["cond"] - 1).abs().max()) < 1e-10
    # the gradients: dense autograd, off-diagonal blocks of gA dropped
    Ad, bd, igd = (t.clone().requires_grad_(True) for t in (torch.block_diag(*A), b, ig))
    diag = z[:, None] ** delays[None, :] * igd[None, :]
    if absorb:
        diag = diag * igz
    T = torch.diag_embed(diag) - (Ad.T if transpose else Ad).to(ref.C128)[None]
    Y = torch.linalg.solve(T, bd.to(ref.C128)[None, :, None].expand(K, N, 1)).squeeze(-1)
    (Y.real * gY.real + Y.imag * gY.imag).sum().backward()
    gA = torch.stack([Ad.grad[i * nper:(i + 1) * nper, i * nper:(i + 1) * nper] for i in range(nblk)])
    for got, want in ((r["gA"], gA), (r["gb"], bd.grad), (r["gig"], igd.grad)):
        assert float((got - want).abs().max() / want.abs().max()) < 1e-12
    # a bin's error is seen on the bin's own scale: one entry of an ordinary bin off by 1e-3 of that bin
    k = int(r["Y"].abs().max(1).values.argmin())
    Yw = r["Y"].clone()
    Yw[k, 0] += 1e-3 * r["Y"][k].abs().max()
    assert ref.per_bin_err(Yw, r) == pytest.approx(1e-3 / float(r["cond"][k]), rel=1e-6)


def test_dispatch_rule_and_coverage(hip_ops):
    from tests import test_gpu_solve_paths as cases
    cases.every_path_is_covered(hip_ops)
    with pytest.raises(RuntimeError, match="unsupported size"):
        hip_ops.solve_path(1, 33)
    with pytest.raises(RuntimeError, match="bad argument"):
        hip_ops.solve_path(0, 4)
    with pytest.raises(RuntimeError, match="unsupported size"):
        hip_ops.solve_phi_path(9, 1)
    # the thread-per-system backward of 5 .. 8 lines needs the saved solution
    assert hip_ops.solve_path(4, 8, backward=True, have_Y=False) == ("generic8", False)
    assert hip_ops.solve_path(4, 8, backward=True, have_Y=True) == ("solve8", False)
    assert hip_ops.solve_path(4, 8, precise=True, backward=True, have_Y=True) == ("generic8", True)
