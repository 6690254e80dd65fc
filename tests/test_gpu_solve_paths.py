"""Every dispatch path of the resolvent solve (csrc/solve.hip) against the float64 reference of tests/solve_ref.py.

The launchers pick one of ten kernel families (and a float64 instantiation of four of them) from (nblk, nper, precise,
saved Y); ``hip_ops.solve_path`` / ``solve_phi_path`` report the choice, and every case here asserts that it runs the
family it names -- a threshold that moves fails ``test_every_path_is_covered`` instead of silently un-testing a kernel.
Shapes are the smallest that reach a path: K in {1, 7, 257}, block counts at and next to the table limits, block counts
that do not divide the workgroup, and per family one K read from the constants of the source at which the number of
partial-sum slots is clamped (a workgroup then walks more than one chunk of bins).

Two metrics per solution:
  (a) ``rel_err``, largest error over largest entry of the whole (K, N) result: 2e-5 (float32 kernels), 1e-6 (precise);
      gradients 1e-4 / 1e-5.  The project's bounds.
  (b) ``per_bin_err``: every bin on its own scale, divided by the bin's float64 condition number, largest over the bins.
      A resolvent has resonant peaks; a wrong bin of ordinary size away from a peak is far below 2e-5 of the peak and
      passes (a).  The bounds are four times the worst value measured per family on an MI355X against the float64
      reference (PERBIN below); for scale, n eps_f32 = 32 * 6e-8 = 2e-6 is what backward-stable float32 elimination
      of a 32-line system promises in these units.

Input conditions (asserted per case): float32 cases keep the largest condition number over the bins below 1e3 (prime
delays 640..1600, T60 = 0.8 s at 32 kHz, ortho_param blocks: 3..20 measured, up to 430 with the absorption factors of
modulus 1..1.3 on a lossless line).  The precise cases take the nearly lossless systems of test_precise_solve
(orthogonal blocks, delays 800..4000 at 48 kHz, 1 / gamma in float64) on a grid refined around a resonance, and their
largest condition number lies in 1e3..1e5, both ends asserted (1500..2750 measured).  That range needs T60 = 300 s:
with an orthogonal A, sigma_min(D - A) >= min 1/gamma - 1 = 800 * 3 ln 10 / (48000 T60), so at test_precise_solve's
T60 = 30 s no bin on the unit circle can pass 2.02 / 0.00385 = 525 (285 is the largest a scan finds).
The inputs are rounded to the kernels' formats before both sides see them: input rounding is not part of the error.

Run time on an MI355X: 65 s for the module (827 cases), 9 s of it the float64 references; each is built once, by the
module-scoped ``refs`` fixture, and the slowest case (generic4 clamp, 65 blocks x 16385 bins) takes 1.4 s."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import gfdn_oracle as orc
from tests import solve_ref as ref
from tests.helpers import rel_err
from tests.margins import within

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    for fn in ("include/diffgfdn_hip.h", "diffgfdn_amd/csrc/solve.hip"):
        m = re.search(r"^#define\s+%s\s+(\d+)" % name, open(os.path.join(ROOT, fn)).read(), flags=re.M)
        if m:
            return int(m.group(1))
    raise KeyError(name)


PARTIAL_BLOCKS = _define("GFDN_PARTIAL_BLOCKS")      # partial-sum slots of the lane-parallel backward kernels
S4_MAX_PARTS = _define("S4_MAX_PARTS")               # ... of the thread-per-system backward kernels
S4_MAXBLK, S8_MAXBLK = _define("S4_MAXBLK"), _define("S8_MAXBLK")
RL_R = _define("RL_R")


def _np(n):
    return 4 if n <= 4 else 8 if n <= 8 else 16 if n <= 16 else 32


def _spb(family, nper):
    """bins per workgroup of a lane-parallel family (solve_path_spb of solve.hip)"""
    if family == "rl9":
        return 4 * (64 // ((9 + RL_R - 1) // RL_R))
    if family.startswith("pk"):
        return 4 * (64 // nper)
    return 256 // _np(nper)


def _clamp_K(family, nper):
    """the smallest K whose backward wants more partial-sum slots than it gets: one more workgroup than the clamp"""
    return PARTIAL_BLOCKS * _spb(family, nper) + 1


# metric (b): 4 x the worst per-bin error / condition number measured on an MI355X over this module's cases against the
# float64 reference (the measured value beside each bound).  solve4 stands apart: with one line per block the system is
# 1 x 1, its matrix condition number is 1 whatever the cancellation in z^m / Gamma - a (worst at the absorption cases)
PERBIN = {
    "solve4": 4 * 8.22e-7,                # 8.219e-07  solve4-1-1-257-False-absorb
    "solve8": 4 * 1.51e-7,                # 1.503e-07  solve8-1-5-257-False-logr
    "rl9": 4 * 1.38e-7,                   # 1.375e-07  clamp rl9-1-9-21505
    "pk10": 4 * 1.60e-7,                  # 1.594e-07  pk10-1-10-7-False-plain
    "pk11": 4 * 1.44e-7,                  # 1.438e-07  pk11-1-11-7-False-plain
    "pk12": 4 * 1.55e-7,                  # 1.541e-07  pk12-3-12-7-False-logr
    "generic4": 4 * 1.01e-7,              # 1.010e-07  generic4-65-4-257-True-absorb_logr
    "generic8": 4 * 1.64e-7,              # 1.636e-07  generic8-33-8-7-True-plain
    "generic16": 4 * 1.49e-7,             # 1.481e-07  generic16-2-16-7-False-plain
    "generic32": 4 * 1.98e-7,             # 1.980e-07  generic32-1-17-7-True-logr
    "precise/generic4": 4 * 2.87e-8,      # 2.867e-08  precise clamp 1-4-16385  (the rounding of Y to complex64
                                          #            over condition numbers of 1..2700: smaller where they are large)
    "precise/generic8": 4 * 1.10e-8,      # 1.099e-08  precise clamp 1-8-8193
    "precise/generic16": 4 * 4.92e-9,     # 4.915e-09  precise clamp 1-16-4097
    "precise/generic32": 4 * 2.92e-9,     # 2.913e-09  precise clamp 1-24-2049
    "phi/generic4": 4 * 2.31e-7,          # 2.310e-07  phi clamp 1-4
    "phi/generic8": 4 * 1.33e-7,          # 1.321e-07  phi 1-8-7-False
    "phi/generic16": 4 * 1.47e-7,         # 1.469e-07  phi 3-4-257-True, radius 1.0003
    "phi/generic32": 4 * 1.69e-7,         # 1.683e-07  phi 8-4-257-False, radius 1.0003
}
TOL_Y, TOL_G = 2e-5, 1e-4                 # float32 kernels
TOL_Y64, TOL_G64 = 1e-6, 1e-5             # precise
COND_CAP, COND_CAP64 = 1e3, 1e5
COND_FLOOR64 = 1e3                        # precise: the largest condition number of a case lies in 1e3..1e5

# family -> (nblk, nper): the smallest shapes that reach it
SHAPES = {
    "solve4": [(nblk, nper) for nper in (1, 3, 4) for nblk in (1, 5, S4_MAXBLK)],
    "generic4": [(S4_MAXBLK + 1, 3), (S4_MAXBLK + 1, 4)],
    "solve8": [(nblk, nper) for nper in (5, 8) for nblk in (1, 3, 7, S8_MAXBLK)],
    "generic8": [(S8_MAXBLK + 1, 5), (S8_MAXBLK + 1, 8)],
    "rl9": [(1, 9), (3, 9)],
    "pk10": [(1, 10), (3, 10)],
    "pk11": [(1, 11), (3, 11)],
    "pk12": [(1, 12), (3, 12)],
    "generic16": [(1, 13), (2, 13), (1, 16), (2, 16)],
    "generic32": [(1, 17), (2, 17), (1, 27), (2, 27), (1, 32), (2, 32)],
}
KS = (1, 7, 257)
MODES = ("plain", "logr", "absorb")       # unit circle / radius 1.0003 / per-bin absorption on the unit circle
                                          # ("absorb_logr": absorption at radius 1.0003, one shape per family below)
RADIUS = 1.0003
CASES = [(fam, nblk, nper, K, tr, mode) for fam, shapes in SHAPES.items() for nblk, nper in shapes for K in KS
         for tr in (False, True) for mode in MODES]
CASES += [(fam, *shapes[-1], 257, tr, "absorb_logr") for fam, shapes in SHAPES.items() for tr in (False, True)]
# the clamp: (family of the backward without saved Y, nblk, nper, K).  Thread-per-system kernels: solve4_parts() first
# holds the slices at 1024 (more than 1024 sweeps of 256 / nblk bins), then clamps 8-sweep slices to S4_MAX_PARTS.
CLAMP_CASES = [
    ("solve4", S4_MAXBLK, 3, 1024 * (256 // S4_MAXBLK) + 5),                     # 1026 sweeps -> 1024 slices
    ("solve4", S4_MAXBLK, 1, S4_MAX_PARTS * 8 * (256 // S4_MAXBLK) + 1),         # 2049 slices -> S4_MAX_PARTS
    ("generic8", S8_MAXBLK, 5, 1024 * (256 // S8_MAXBLK) + 5),                   # solve8 with Y: 1025 sweeps -> 1024
    ("generic4", S4_MAXBLK + 1, 3, _clamp_K("generic4", 3)),
    ("generic8", 1, 5, _clamp_K("generic8", 5)),
    ("rl9", 1, 9, _clamp_K("rl9", 9)),
    ("pk10", 1, 10, _clamp_K("pk10", 10)),
    ("pk11", 1, 11, _clamp_K("pk11", 11)),
    ("pk12", 1, 12, _clamp_K("pk12", 12)),
    ("generic16", 1, 13, _clamp_K("generic16", 13)),
    ("generic32", 1, 17, _clamp_K("generic32", 17)),
]
PRECISE_CASES = [(nblk, nper, K, tr) for nper in (4, 8, 11, 16, 24) for nblk in (1, 3) for K in (7, 257)
                 for tr in (False, True)]
PRECISE_CLAMP = [(1, nper, _clamp_K("generic", nper)) for nper in (4, 8, 16, 24)]
# filter coupling: one dense system of N = G nper lines per bin; N > GFDN_MAX_BLOCK is refused
PHI_SHAPES = [(G, nper) for nper in (4, 8, 9, 16) for G in (1, 3, 8)] + [(1, 17), (2, 17)]
PHI_OK = [(G, nper) for G, nper in PHI_SHAPES if G * nper <= 32]
PHI_REFUSED = [(G, nper) for G, nper in PHI_SHAPES if G * nper > 32]
PHI_CASES = [(G, nper, K, absorb, False) for G, nper in PHI_OK for K in KS for absorb in (False, True)]
PHI_CASES += [(G, nper, 257, absorb, True) for G, nper in PHI_OK for absorb in (False, True)]      # radius 1.0003
PHI_CLAMP = [(1, 4), (1, 8), (1, 16), (1, 17)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffgfdn_amd import hip_ops
    return hip_ops


def _prime_table():
    import sympy as sp
    return np.array(list(sp.primerange(640, 1600)), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def float32_inputs(nblk, nper):
    """the recipe of test_solve_fwd_bwd: prime delays 640..1600 (distinct inside a block), T60 = 0.8 s at 32 kHz,
    ortho_param blocks; everything rounded to float32"""
    g = torch.Generator().manual_seed(1000 * nblk + nper)
    rng = np.random.RandomState(1000 * nblk + nper)
    primes = _prime_table()
    delays = torch.tensor(np.concatenate([rng.choice(primes, nper, replace=False) for _ in range(nblk)]))
    ig = ref.f32(10.0 ** (3.0 * delays / (32000 * 0.8)))
    M = torch.randn(nblk, nper, nper, generator=g, dtype=torch.float64) / np.sqrt(nper)
    A = ref.f32(torch.stack([orc.ortho_param(M[i]) for i in range(nblk)]))
    b = ref.f32(torch.randn(nblk * nper, generator=g, dtype=torch.float64) / (nblk * nper))
    return A, delays, ig, b


PRECISE_T60 = 300.0        # seconds: what puts the resonances of these systems at condition numbers of 1e3..1e5
PRECISE_STEP = 2e-7        # radians between the bins of the refined grid (a resonance is about 5e-7 wide)


@functools.lru_cache(maxsize=None)
def precise_inputs(nblk, nper):
    """the systems of test_precise_solve: orthogonal blocks, delays 800..4000 at 48 kHz, 1 / gamma in float64 -- with
    T60 = 300 s (see the module docstring)"""
    g = torch.Generator().manual_seed(7 * nper + nblk)
    A = ref.f32(torch.stack([torch.linalg.qr(torch.randn(nper, nper, generator=g, dtype=torch.float64))[0]
                             for _ in range(nblk)]))
    delays = torch.randint(800, 4000, (nblk * nper,), generator=g).to(torch.float64)
    ig = 10.0 ** (3.0 * delays / (48000.0 * PRECISE_T60))
    b = ref.f32(torch.randn(nblk * nper, generator=g, dtype=torch.float64))
    return A, delays, ig, b


@functools.lru_cache(maxsize=None)
def precise_peak(nblk, nper):
    """angle of a resonance of block 0: the worst-conditioned bin of a scan, 1e-7 rad apart, over one and a half times
    the mean distance of the block's poles (2 pi / sum of its delays) from 1 rad on"""
    A, delays, ig, _ = precise_inputs(nblk, nper)
    d0, ig0 = delays[:nper], ig[:nper]
    npts = int(1.5 * 2 * np.pi / float(d0.sum()) / 1e-7) + 1
    theta = 1.0 + 1e-7 * torch.arange(npts, dtype=torch.float64)
    z = torch.exp(1j * theta).to(ref.C128)
    T = torch.diag_embed(z[:, None] ** d0[None, :] * ig0[None, :]) - A[0].to(ref.C128)[None]
    s = torch.linalg.svdvals(T)
    return float(theta[int((s[:, 0] / s[:, -1]).argmax())])


def precise_grid(nblk, nper, K):
    """K bins on the unit circle, PRECISE_STEP apart, the middle one on the resonance"""
    theta = precise_peak(nblk, nper) + PRECISE_STEP * (torch.arange(K, dtype=torch.float64) - K // 2)
    return torch.exp(1j * theta).to(ref.C128)


def _cotangent(K, N, seed):
    g = torch.Generator().manual_seed(seed)
    return ref.c64(torch.view_as_complex(torch.randn(K, N, 2, generator=g, dtype=torch.float64)))


def _absorption(K, N, seed):
    """1 / Gamma_i(z_k): modulus 1..1.3, random phase, complex64"""
    g = torch.Generator().manual_seed(seed + 1)
    mod = 1.0 + 0.3 * torch.rand(K, N, generator=g, dtype=torch.float64)
    return ref.c64(torch.polar(mod, 2 * np.pi * torch.rand(K, N, generator=g, dtype=torch.float64)))


def reference(nblk, nper, K, transpose, mode, precise=False):
    """(z, igz, gY, float64 reference) of one case"""
    A, delays, ig, b = (precise_inputs if precise else float32_inputs)(nblk, nper)
    N = nblk * nper
    seed = 31 * K + 2 * N + int(transpose)
    z = (precise_grid(nblk, nper, K) if precise else ref.grid(K)) * (RADIUS if mode.endswith("logr") else 1.0)
    igz = _absorption(K, N, seed) if mode.startswith("absorb") else None
    gY = _cotangent(K, N, seed)
    r = ref.solve_ref(z, delays, torch.ones_like(ig) if igz is not None else ig, A, b, transpose, igz, gY)
    return z, igz, gY, r


def _d(t):
    return None if t is None else t.to(DEV)


@pytest.fixture(scope="module")
def refs():
    """the float64 references of the module, each built once (a case that runs again, or shares its system with
    another test, finds it here) and left unchanged"""
    built = {}

    def get(fn, *key):
        if (fn, key) not in built:
            built[(fn, key)] = fn(*key)
        return built[(fn, key)]
    return get


def check_solve(ops, refs, family, nblk, nper, K, transpose, mode, precise=False):
    """forward, backward without and with the saved solution, each on the family it must run and inside both metrics"""
    A, delays, ig, b = (precise_inputs if precise else float32_inputs)(nblk, nper)
    z, igz, gY, r = refs(reference, nblk, nper, K, transpose, mode, precise)
    cap, tol_y, tol_g = (COND_CAP64, TOL_Y64, TOL_G64) if precise else (COND_CAP, TOL_Y, TOL_G)
    assert float(r["cond"].max()) < cap, ("input condition", float(r["cond"].max()))
    if precise:
        assert float(r["cond"].max()) >= COND_FLOOR64, ("input condition", float(r["cond"].max()))
    fwd_family = ops.solve_path(nblk, nper, precise, False, False)
    bwd_family = ops.solve_path(nblk, nper, precise, False, True)
    bwd_saved = ops.solve_path(nblk, nper, precise, True, True)
    if family == "solve8":                   # the thread-per-system backward needs the saved solution
        assert (fwd_family, bwd_family, bwd_saved) == (("solve8", False), ("generic8", False), ("solve8", False))
    else:
        assert fwd_family == bwd_family == bwd_saved == (family, precise)
    turns, logr = ops.zprep(z.to(DEV))
    logr = logr if mode.endswith("logr") else None
    if igz is not None:
        ig = torch.ones_like(ig)
    args = (turns, logr, _d(A), _d(delays), _d(ig), _d(b))
    Y = ops.solve_fwd(*args, transpose, inv_gamma_bins=_d(igz), precise=precise)
    tag = "precise/" if precise else ""
    assert rel_err(Y.cpu(), r["Y"]) < tol_y
    within(ref.per_bin_err(Y, r), PERBIN[tag + fwd_family[0]], "perbin/" + tag + fwd_family[0])
    for saved in (None, Y):
        gA, gb, gig = ops.solve_bwd(*args, _d(gY), transpose, Y=saved, inv_gamma_bins=_d(igz), precise=precise)
        assert rel_err(gA.cpu(), r["gA"]) < tol_g, ("gA", saved is not None)
        assert rel_err(gb.cpu(), r["gb"]) < tol_g, ("gb", saved is not None)
        if igz is None:                      # (the absorption filters are fixed: no gradient w.r.t. them)
            assert rel_err(gig.cpu(), r["gig"]) < tol_g, ("gig", saved is not None)


@pytest.mark.parametrize("family,nblk,nper,K,transpose,mode", CASES)
def test_solve_path(ops, refs, family, nblk, nper, K, transpose, mode):
    check_solve(ops, refs, family, nblk, nper, K, transpose, mode)


@pytest.mark.parametrize("bwd_family,nblk,nper,K", CLAMP_CASES)
def test_solve_partial_clamp(ops, refs, bwd_family, nblk, nper, K):
    """K past the partial-sum slots: the backward's workgroups walk more than one chunk of bins"""
    family = ops.solve_path(nblk, nper, False, True, True)[0]
    assert ops.solve_path(nblk, nper, False, False, True)[0] == bwd_family
    clamped = False
    if bwd_family != "solve4":               # lane-parallel without the saved solution
        want = -(-K // _spb(bwd_family, nper))
        clamped = want > PARTIAL_BLOCKS and want % PARTIAL_BLOCKS != 0
    if family in ("solve4", "solve8"):       # thread-per-system (with the saved solution): solve4_parts() of solve.hip
        rows = 256 // nblk
        sweeps, slices = -(-K // rows), -(-K // (8 * rows))
        clamped |= slices < 1024 < sweeps and sweeps % 1024 != 0
        clamped |= slices > S4_MAX_PARTS and slices % S4_MAX_PARTS != 0
    assert clamped, "K does not cross a clamp of this shape"
    check_solve(ops, refs, family, nblk, nper, K, False, "plain")


@pytest.mark.parametrize("nblk,nper,K,transpose", PRECISE_CASES)
def test_precise_path(ops, refs, nblk, nper, K, transpose):
    check_solve(ops, refs, "generic%d" % _np(nper), nblk, nper, K, transpose, "plain", precise=True)


@pytest.mark.parametrize("nblk,nper,K", PRECISE_CLAMP)
def test_precise_partial_clamp(ops, refs, nblk, nper, K):
    assert -(-K // (256 // _np(nper))) == PARTIAL_BLOCKS + 1
    check_solve(ops, refs, "generic%d" % _np(nper), nblk, nper, K, False, "plain", precise=True)


# ---- filter coupling ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def phi_inputs(G, nper):
    """the model's structure: BM[(i,a),(j,c)] = (Q_i Q_j)[a,c] with ortho_param rotations Q_g; with a unitary Phi_k the
    feedback matrix BM o kron(Phi_k, 1) is unitary and the system as well conditioned as the uncoupled ones"""
    N = G * nper
    g = torch.Generator().manual_seed(100 * G + nper)
    rng = np.random.RandomState(100 * G + nper)
    delays = torch.tensor(rng.choice(_prime_table(), N, replace=False))
    ig = ref.f32(10.0 ** (3.0 * delays / (32000 * 0.8)))
    Q = torch.stack([orc.ortho_param(torch.randn(nper, nper, generator=g, dtype=torch.float64) / np.sqrt(nper))
                     for _ in range(G)])
    BM = ref.f32(torch.einsum("iab,jbc->iajc", Q, Q).reshape(N, N))
    b = ref.f32(torch.randn(N, generator=g, dtype=torch.float64) / N)
    U = [orc.ortho_param(torch.randn(G, G, generator=g, dtype=torch.float64)).to(ref.C128) for _ in range(2)]
    return BM, delays, ig, b, U


def phi_reference(G, nper, K, absorb, off_circle=False):
    BM, delays, ig, b, U = phi_inputs(G, nper)
    N = G * nper
    z = ref.grid(K) * (RADIUS if off_circle else 1.0)
    # a unitary, frequency-dependent coupling: U0 diag(z^-p) U1, p = 0 .. G-1  (a paraunitary FIR matrix on the grid)
    zp = (z / z.abs())[:, None] ** (-torch.arange(G, dtype=torch.float64))[None, :]
    Phi = ref.c64(U[0][None] @ torch.diag_embed(zp) @ U[1][None])
    seed = 17 * K + N
    igz = _absorption(K, N, seed) if absorb else None
    gY = _cotangent(K, N, seed)
    return z, Phi, igz, gY, ref.solve_phi_ref(z, delays, ig, BM, Phi, nper, b, igz, gY)


def check_phi(ops, refs, G, nper, K, absorb, off_circle=False):
    BM, delays, ig, b, _ = phi_inputs(G, nper)
    z, Phi, igz, gY, r = refs(phi_reference, G, nper, K, absorb, off_circle)
    assert float(r["cond"].max()) < COND_CAP, ("input condition", float(r["cond"].max()))
    family, precise = ops.solve_phi_path(G, nper)
    assert (family, precise) == ("generic%d" % _np(G * nper), False)
    turns, logr = ops.zprep(z.to(DEV))
    args = (turns, logr if off_circle else None, _d(BM), _d(Phi), nper, _d(delays), _d(ig), _d(b))
    Y = ops.solve_phi_fwd(*args, inv_gamma_bins=_d(igz))
    assert rel_err(Y.cpu(), r["Y"]) < TOL_Y
    within(ref.per_bin_err(Y, r), PERBIN["phi/" + family], "perbin/phi/" + family)
    gBM, gb, gig, gPhi = ops.solve_phi_bwd(*args, _d(gY), Y, inv_gamma_bins=_d(igz))
    for name, got in (("gBM", gBM), ("gb", gb), ("gig", gig), ("gPhi", gPhi)):
        assert rel_err(got.cpu(), r[name]) < TOL_G, name


@pytest.mark.parametrize("G,nper,K,absorb,off_circle", PHI_CASES)
def test_solve_phi_path(ops, refs, G, nper, K, absorb, off_circle):
    check_phi(ops, refs, G, nper, K, absorb, off_circle)


@pytest.mark.parametrize("G,nper", PHI_CLAMP)
def test_solve_phi_partial_clamp(ops, refs, G, nper):
    K = _clamp_K("generic", G * nper)
    assert -(-K // (256 // _np(G * nper))) == PARTIAL_BLOCKS + 1
    check_phi(ops, refs, G, nper, K, True)


@pytest.mark.parametrize("G,nper", PHI_REFUSED)
def test_solve_phi_refuses_what_it_cannot_run(ops, G, nper):
    """more than GFDN_MAX_BLOCK lines (nper = 17 with two groups among them): GFDN_E_UNSUPPORTED from the query and from
    both launchers, raised through _lib.check -- never a return of 0 without a launch"""
    N, K = G * nper, 7
    with pytest.raises(RuntimeError, match="unsupported size"):
        ops.solve_phi_path(G, nper)
    z = ref.grid(K)
    turns, _ = ops.zprep(z.to(DEV))
    BM = torch.eye(N, device=DEV)
    Phi = torch.ones(K, G, G, dtype=torch.complex64, device=DEV)
    v = torch.ones(N, device=DEV)
    Y = torch.zeros(K, N, dtype=torch.complex64, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported size"):
        ops.solve_phi_fwd(turns, None, BM, Phi, nper, 2 * v, 2 * v, v)
    with pytest.raises(RuntimeError, match="unsupported size"):
        ops.solve_phi_bwd(turns, None, BM, Phi, nper, 2 * v, 2 * v, v, Y, Y)


# ---- coverage ----------------------------------------------------------------------------------------------------
def every_path_is_covered(ops):
    """the parameter lists above reach every kernel family, forward and backward, float32 and float64, and all four
    lane counts of the filter-coupled launchers (host-side queries only: tests/test_solve_ref.py runs it without a
    GPU)"""
    fwd, bwd, phi = set(), set(), set()
    plain = [(c[1], c[2], False) for c in CASES] + [(c[1], c[2], False) for c in CLAMP_CASES]
    prec = [(c[0], c[1], True) for c in PRECISE_CASES] + [(c[0], c[1], True) for c in PRECISE_CLAMP]
    for nblk, nper, precise in plain + prec:
        fwd.add(ops.solve_path(nblk, nper, precise, False, False))
        for have_Y in (False, True):
            bwd.add(ops.solve_path(nblk, nper, precise, have_Y, True))
    for G, nper in PHI_OK + PHI_CLAMP:
        phi.add(ops.solve_phi_path(G, nper))
    generic = ["generic4", "generic8", "generic16", "generic32"]
    every = {(f, False) for f in ops.SOLVE_PATHS.values()} | {(f, True) for f in generic}
    assert fwd == every
    assert bwd == every
    assert phi == {(f, False) for f in generic}
    assert set(SHAPES) == set(ops.SOLVE_PATHS.values())
    assert set(PERBIN) == set(SHAPES) | {"precise/" + f for f in generic} | {"phi/" + f for f in generic}
    for family, shapes in SHAPES.items():    # every float32 shape sits under the family it is listed for
        for nblk, nper in shapes:
            assert ops.solve_path(nblk, nper, False, True, True)[0] == family, (family, nblk, nper)


def test_every_path_is_covered(ops):
    every_path_is_covered(ops)


# ---- the trainer's gain normalisation ------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("nper", [1, 4, 9])
def test_normalize_io(ops, G, nper):
    """gfdn_normalize_io: b[n], c[n] /= energy[group(n)]^(1/4) in place (trainer.py:317-332), against float64.  Every
    element on its own scale: powf within 2 ulp, one rounding of the division, 1 ulp of slack = 4 eps_f32."""
    g = torch.Generator().manual_seed(10 * G + nper)
    N = G * nper
    energy = (0.05 + 40.0 * torch.rand(G, generator=g)).to(torch.float32)
    b, c = torch.randn(N, generator=g), torch.randn(N, generator=g)
    s = energy.double().repeat_interleave(nper) ** 0.25
    bk, ck = b.to(DEV), c.to(DEV)
    ops.normalize_io(energy.to(DEV), bk, ck, G, nper)
    for got, want in ((bk, b.double() / s), (ck, c.double() / s)):
        within(float(((got.cpu().double() - want) / want).abs().max()), 4 * 2.0 ** -23, "normalize_io")
