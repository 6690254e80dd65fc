"""Band-parallel driver: one independent GFDN per octave band, bands spread over the GPUs of a node.

Counterpart of the reference's src/run_subband_training_treble.py: ``training`` (:175-204) trains the
bands one after another in one process; ``inferencing`` (:207-375) rebuilds every band's model, renders
the RIRs (``get_response``), filters each with its band's reconstructing FIR (``fftconvolve(h, taps,
'full')``, :321-324) and sums the bands per receiver (:358).

Bands share neither parameters nor data, so on MI355X they are placed on
different ranks with NO collective during training; the only exchange is the final sum over bands
of the filtered RIRs, one ``reduce`` of a (receivers, samples) float32 tensor to rank 0 over
RCCL / xGMI.  FIR taps are an input (the reference takes them from pyfar).
"""
from typing import Callable, Dict, List, Optional, Sequence

import torch
import torch.distributed as dist

from . import hip_ops as ops
from .trainer import get_response


def band_assignment(freqs: Sequence[float], world_size: int) -> List[List[float]]:
    """Round-robin placement of bands on ranks: rank r trains freqs[r::world_size]."""
    return [list(freqs[r::world_size]) for r in range(world_size)]


def train_bands(freqs: Sequence[float], build_band: Callable[[float], tuple], rank: int = 0,
                world_size: int = 1) -> Dict[float, object]:
    """Train this rank's bands one after another (reference ``training``); ``build_band(freq)`` returns
    (trainer, train_loader, valid_loader).  No communication: every band is its own model."""
    trainers = {}
    for f in band_assignment(freqs, world_size)[rank]:
        trainer, train_loader, valid_loader = build_band(f)
        trainer.train(train_loader, valid_loader)
        trainers[f] = trainer
    return trainers


def full_convolve(h: torch.Tensor, taps: torch.Tensor) -> torch.Tensor:
    """scipy.signal.fftconvolve(h[r], taps, mode='full') for every row r, on the library's FFTs:
    zero-pad both to the next power of two >= len(h) + len(taps) - 1, multiply spectra, invert."""
    T, M = h.shape[-1], taps.numel()
    full = T + M - 1
    n = 1 << (full - 1).bit_length()
    Hf = ops.rfft_pow2(h, n)
    Tf = ops.rfft_pow2(taps.reshape(1, -1).to(h.device), n)
    y = ops.irfft_pow2_fwd(Hf * Tf, n)
    return y[..., :full]


@torch.no_grad()
def render_band(net, batches, taps: torch.Tensor) -> torch.Tensor:
    """Filtered RIRs of one band for all batches (reference :308-324): (receivers, nfft + taps - 1)."""
    out = []
    for data in batches:
        h = get_response(data, net)[-1]
        out.append(full_convolve(h.contiguous(), taps))
    return torch.cat(out, dim=0)


@torch.no_grad()
def infer_bands(freqs: Sequence[float], load_band: Callable[[float], tuple], rank: int = 0, world_size: int = 1,
                group=None, dst: int = 0) -> Optional[torch.Tensor]:
    """The reference's ``inferencing`` (:207-375) over the ranks of a job: this rank renders ITS bands
    (``load_band(freq)`` -> (net with the trained state loaded, batches, FIR taps of the band's reconstructing
    filter)), filters them (``render_band``) and the bands are summed per receiver on ``dst`` (``sum_bands``; a rank
    without bands contributes zeros).  Returns the full-band RIRs (receivers, nfft + taps - 1) on ``dst``."""
    local, device = [], None
    for f in band_assignment(freqs, world_size)[rank]:
        net, batches, taps = load_band(f)
        net.eval()
        local.append(render_band(net, batches, taps))
        device = local[-1].device
    return sum_bands(local, group=group, dst=dst, device=device)


@torch.no_grad()
def infer_bank(bank, dataset, taps, rows=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The full-band RIRs of a trained band bank in one pass: what ``infer_bands`` returns for ``bank.nets``, the bands'
    datasets and ``taps`` (the reference's ``inferencing``, :207-375), without leaving the bank.  Neither irfft nor the
    convolution depends on the receiver, which enters only through its G gains per band:

        y[r] = sum_q fftconvolve(irfft(H_q[r]), taps_q) = D[r] + sum_{q,g} gain_q[r][g] (irfft(T_{q,g}) (*) taps_q)

    ``D = dataset.direct_render(taps)`` is a constant of the dataset (built on the first call, cached per taps), the model
    contributes bands x G filtered group signals (``bank.filtered_group_signals``) and all receivers are one product
    Y = D + W C (``hip_ops.render_mix``, csrc/render.hip) with the gains W of ``bank.render_gains``.

    ``bank``: BandBank; ``dataset``: the BandStackedDataset of its bands; ``taps``: (bands, M) tensor or a sequence of
    equal-length tensors; ``rows``: receivers to render, in this order (default: all R) -- a job that spreads the receivers
    over its ranks passes every rank its share, no collective is involved; ``out``: (len(rows) or R, nfft + M - 1) float32
    buffer to fill.  Returns (len(rows) or R, nfft + M - 1) float32 on the bank's device."""
    dev = bank.input_gains.device
    if not torch.is_tensor(taps):
        taps = torch.stack([torch.as_tensor(t) for t in taps])
    taps = taps.detach().to(device=dev, dtype=torch.float32)
    if taps.dim() != 2 or taps.shape[0] != bank.num_bands or dataset.num_bands != bank.num_bands:
        raise ValueError("infer_bank: one row of taps and one dataset per band of the bank")
    taps = taps.contiguous()
    sel = None
    if rows is not None:
        sel = torch.as_tensor(rows, dtype=torch.long, device=dev).reshape(-1).contiguous()
        if sel.numel() == 0 or int(sel.min()) < 0 or int(sel.max()) >= dataset.R:
            raise ValueError("infer_bank: rows must name receivers of the dataset")
    D = dataset.direct_render(taps)
    C = bank.filtered_group_signals(dataset.z_values, taps)
    W = bank.render_gains(dataset.norm_listener_position, dataset.R, sel)
    return ops.render_mix(D, W, C, rows=sel, out=out)


def same_convolve(h: torch.Tensor, taps: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scipy.signal.fftconvolve(h[r], taps, mode='same') for every row r: the L = len(h[r]) samples of the full convolution
    from sample (M - 1) // 2 on (scipy centres the result on its first argument)."""
    L, M = h.shape[-1], taps.numel()
    y = full_convolve(h, taps)[..., (M - 1) // 2:(M - 1) // 2 + L]
    if out is None:
        return y
    out.copy_(y)
    return out


def directional_mix_torch(W: torch.Tensor, C: torch.Tensor, Ls: int, A: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hip_ops.dir_render`` in stock tensor operations, the two-stage formulation: Ls skinny products into the ambisonic
    RIRs of all receivers, then the J x Ls contraction.  For the shapes the kernel does not take (and as its yardstick in
    tools/time_directional_render.py)."""
    R, n = W.shape[0], C.shape[1]
    W3, C3 = W.reshape(R, -1, Ls), C.reshape(-1, Ls, C.shape[1])
    ambi = out if (A is None and out is not None) else torch.empty((R, Ls, n), dtype=torch.float32, device=C.device)
    for l in range(Ls):
        ambi[:, l] = W3[:, :, l] @ C3[:, l]
    if A is None:
        return ambi
    res = torch.matmul(A, ambi)
    if out is None:
        return res
    out.copy_(res)
    return out


def directional_mix(W: torch.Tensor, C: torch.Tensor, Ls: int, A: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(R, J or Ls, n): the receivers' directional (``A`` (J, Ls) given) or ambisonic RIRs from their SH weights W (R, S, Ls)
    and the filtered signals C (S Ls, n): ``hip_ops.dir_render`` (csrc/dirrender.hip) within its limits (S <= 32, Ls <= 16,
    J <= 32), the same result from ``directional_mix_torch`` beyond them."""
    S = C.shape[0] // Ls
    if (S > ops.DIR_RENDER_MAX_S or Ls > ops.DIR_RENDER_MAX_LS
            or (A is not None and A.shape[0] > ops.DIR_RENDER_MAX_J)):
        return directional_mix_torch(W, C, Ls, A, out)
    return ops.dir_render(W, C, Ls, a=A, out=out)


def directional_band_signals(nets, z_values: torch.Tensor, taps: torch.Tensor, length: int) -> torch.Tensor:
    """C (Q G Ls, length): per band q and delay line n = g Ls + l the line's response with its output gain, c_n Y_q[:, n],
    brought to the time domain (irfft, n = 2 (K - 1)), cut to ``length`` and through the band's reconstructing FIR
    (``same_convolve``) -- Q G Ls signals whatever the number of receivers.  The cut comes before the filter, as in the
    reference (inference.py:479-481, then :807-810).  The rows' pitch is a multiple of four samples."""
    K = z_values.shape[-1]
    nfft = 2 * (K - 1)
    if nfft < 16 or nfft & (nfft - 1):
        raise ValueError("directional_band_signals: the frequency grid of a power-of-two transform (K = nfft / 2 + 1)")
    N = nets[0].num_groups * nets[0].num_delay_lines_per_group
    C = torch.empty((len(nets) * N, (length + 3) // 4 * 4), dtype=torch.float32, device=z_values.device)[:, :length]
    for q, net in enumerate(nets):
        net.feedback_loop.new_forward()
        Y = net.delay_line_responses(z_values, transpose=True)                     # (K, N)
        X = (Y * net.output_gains.reshape(1, -1)).transpose(0, 1).contiguous()     # (N, K)
        h = ops.irfft_pow2_fwd(X, nfft)[:, :length]
        same_convolve(h.contiguous(), taps[q], out=C[q * N:(q + 1) * N])
    return C


@torch.no_grad()
def infer_directional_bands(nets, z_values, norm_listener_position, taps, length: int, directional: bool = True, rows=None,
                            out: Optional[torch.Tensor] = None, chunk: int = 4096) -> torch.Tensor:
    """The spatial RIRs of all receivers from the trained directional bands in one pass: what the reference's
    ``infer_all_octave_bands_directional_fdn`` (inference.py:676-881, with ``InferDiffDirectionalFDN.get_model_output``
    :402-481) builds band by band and receiver by receiver -- get_response (h = irfft(H_sh), n = 2 (K - 1)), the cut to
    ``edc_len_samps``, optionally the conversion to directional RIRs with the analysis matrix (:387-400),
    fftconvolve(.., mode='same') with the band's reconstructing FIR (:807-810), the sum over the bands per receiver
    (:837-862).  Neither the inverse transform, the cut nor the FIR depends on the receiver, which enters only through its
    G x (order+1)^2 SH weights per band (``sh_output_scalars`` with normalised weights):

        C[q][g][l]    = same_conv(irfft(c_{g,l} Y_q[:, g Ls + l], n = 2 (K - 1))[:length], taps_q)     Q G Ls signals
        ambi[r][l][t] = sum_{q,g} w_q[r][g][l] C[q][g][l][t]                                        (directional=False)
        dir[r][j][t]  = sum_l A[j][l] ambi[r][l][t]                                                 (directional=True)

    (conversion and band sum are linear: converting after the sum is the reference's convert-then-sum up to rounding).
    All receivers are ONE launch of ``hip_ops.dir_render`` (csrc/dirrender.hip), the ambisonic RIRs never stored in the
    directional mode; beyond the kernel's limits (Q G > 32, more than 16 channels or 32 directions) the same result comes
    from stock tensor operations (``directional_mix_torch``).

    ``nets``: the Q trained DiffDirectionalFDNVarReceiverPos models, one per band, with the same G, order and analysis
    matrix; ``z_values`` (K,) the frequency grid, K = 2^p + 1; ``norm_listener_position`` (R, 3) the receivers' normalised
    positions; ``taps`` (Q, M) the bands' reconstructing FIRs; ``length``: the reference's ``edc_len_samps``, clamped to
    2 (K - 1); ``directional=False`` is the reference's ``sum_ambi_directly=True``; ``rows``: receivers to render, in this
    order (default: all R); ``out``: a (len(rows) or R, J or Ls, length) float32 view to fill; ``chunk``: positions per
    evaluation of a band's weight network.  Returns (len(rows) or R, J or (order+1)^2, length) float32.

    Not covered: ``apply_filter_norm`` (the reference's driver passes False), the conversion of the summed directional RIRs
    back to ambisonics (:864-881, spaudiopy), the checkpoints and per-band pickles the reference reads and writes on the
    way.  Binaural rendering (sound_examples.py:356-535), which consumes this function's result, is
    ``render_binaural_moving_listener_bands`` (from the bands, in one pass) and ``render_binaural_moving_listener``."""
    W, C, Ls, A = _directional_inputs(nets, z_values, norm_listener_position, taps, length, rows, chunk,
                                      "infer_directional_bands")
    return directional_mix(W, C, Ls, A if directional else None, out)


def _directional_inputs(nets, z_values, norm_listener_position, taps, length: int, rows, chunk: int, what: str):
    """the band checks of ``infer_directional_bands`` and what its mix takes: (W (R, Q G, Ls) the receivers' normalised SH
    weights, C (Q G Ls, L) the filtered band signals, Ls, the analysis matrix)"""
    nets = list(nets)
    if not nets:
        raise ValueError(f"{what}: no bands")
    dev = nets[0].output_gains.device
    G, Ls = nets[0].num_groups, nets[0].num_delay_lines_per_group
    A = nets[0].sh_output_scalars.analysis_matrix
    for net in nets[1:]:
        An = net.sh_output_scalars.analysis_matrix
        if (net.num_groups != G or net.num_delay_lines_per_group != Ls or An.shape != A.shape
                or not torch.equal(An.to(A.device), A)):
            raise ValueError(f"{what}: the bands must share groups, order and analysis matrix")
    if not torch.is_tensor(taps):
        taps = torch.stack([torch.as_tensor(t) for t in taps])
    taps = taps.detach().to(device=dev, dtype=torch.float32).contiguous()
    if taps.dim() != 2 or taps.shape[0] != len(nets) or taps.shape[1] < 1:
        raise ValueError(f"{what}: one row of taps per band")
    pos = norm_listener_position.detach().to(device=dev, dtype=torch.float32).reshape(-1, 3)
    if rows is not None:
        sel = _edc_rows(rows, pos.shape[0], dev, what)
        pos = pos[sel]
    z = z_values.to(dev)
    L = max(1, min(int(length), 2 * (z.shape[-1] - 1)))
    C = directional_band_signals(nets, z, taps, L)
    R = pos.shape[0]
    W = torch.empty((R, len(nets), G, Ls), dtype=torch.float32, device=dev)
    for q, net in enumerate(nets):
        for r0 in range(0, R, int(chunk)):
            W[r0:r0 + chunk, q] = net.sh_output_scalars({'norm_listener_position': pos[r0:r0 + chunk]},
                                                        normalise_weights=True)
    return W.view(R, len(nets) * G, Ls), C, Ls, A.to(dev)


def band_split(x: torch.Tensor, analysis_taps: torch.Tensor, length: int, chunk: int = 32,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(rows, A, length) float32: the first ``length`` samples of ``full_convolve(x[r], analysis_taps[k])`` for every row
    and analysis band -- the reference's ``octave_filtering`` (plot.py:632-661) with the filterbank as a declared input:
    causal FIRs, THE FIRST ``length`` SAMPLES OF THE CAUSAL CONVOLUTION (truncating before or after the filter is the
    same).  x (rows, T) float32 on the device, analysis_taps (A, Ma).  One forward transform per row, one inverse per row
    and band, ``chunk`` rows at a time (bounded temporaries).  The rows' pitch is a multiple of four samples
    (csrc/edcerr.hip moves them 16 bytes per lane); ``out``: any (rows, A, length) float32 view to fill instead."""
    length = int(length)
    if x.dim() != 2 or analysis_taps.dim() != 2 or length < 1 or x.shape[1] < 1:
        raise ValueError("band_split: x (rows, T), analysis_taps (A, Ma), length >= 1")
    at = analysis_taps.detach().to(device=x.device, dtype=torch.float32).contiguous()
    A, Ma = at.shape
    T = min(x.shape[1], length)
    n = max(16, 1 << (T + Ma - 2).bit_length())
    m = min(length, n)
    if out is None:
        out = ops.empty_bands(x.shape[0], A, length, x.device)
    elif tuple(out.shape) != (x.shape[0], A, length) or out.dtype != torch.float32:
        raise ValueError("band_split: out (rows, A, length) float32")
    if m < length:
        out[:, :, m:] = 0.0                               # (behind the end of the full convolution)
    Tf = ops.rfft_pow2(at, n)
    for r0 in range(0, x.shape[0], chunk):
        Xf = ops.rfft_pow2(x[r0:r0 + chunk, :T], n)
        for k in range(A):
            out[r0:r0 + chunk, k, :m] = ops.irfft_pow2_fwd(Xf * Tf[k], n)[:, :m]
    return out


def _edc_taps(bank, taps, analysis_taps):
    dev = bank.input_gains.device
    if not torch.is_tensor(taps):
        taps = torch.stack([torch.as_tensor(t) for t in taps])
    if taps.device != dev or taps.dtype != torch.float32 or not taps.is_contiguous():
        taps = taps.detach().to(device=dev, dtype=torch.float32).contiguous()
    if analysis_taps is None:
        return taps, taps
    if not torch.is_tensor(analysis_taps):
        analysis_taps = torch.stack([torch.as_tensor(t) for t in analysis_taps])
    if analysis_taps.device != dev or analysis_taps.dtype != torch.float32 or not analysis_taps.is_contiguous():
        analysis_taps = analysis_taps.detach().to(device=dev, dtype=torch.float32).contiguous()
    return taps, analysis_taps


def _edc_rows(rows, R: int, dev, what: str):
    """``rows`` as a checked int64 device vector; host data is checked on the host (no device sync)"""
    if rows is None:
        return None
    sel = torch.as_tensor(rows, dtype=torch.long).reshape(-1)
    if sel.numel() == 0 or int(sel.min()) < 0 or int(sel.max()) >= R:
        raise ValueError(f"{what}: rows must name receivers of the dataset")
    return sel.to(dev).contiguous()


def _rmse(err: torch.Tensor) -> torch.Tensor:
    return torch.linalg.vector_norm(err, dim=0) / float(err.shape[0]) ** 0.5


@torch.no_grad()
def edc_error_bank(bank, dataset, taps, measured, sample_rate: Optional[float] = None, analysis_taps=None, rows=None):
    """The EDC matching error of a trained band bank over the receiver grid in one pass: the reference's
    ``plot_edc_error_in_space`` -> ``get_edc_error`` (plot.py:606-757, the metric at :632-661; its "RMSE in matching EDC at
    ... Hz is ... dB" line) of the bank's full-band render (``infer_bank``) against the measured RIRs.

        L = min(Tx, Ty, int(2 sample_rate))                                                     (plot.py:689-694)
        x_k[r] = (a_k * measured[r])[:L],  y_k[r] = (a_k * y[r])[:L]        a_k = analysis_taps[k], causal convolution
        E_k[r][t] = sum_{u >= t} x_k[r][u]^2, likewise for y     (normalize = False, discard_last_zeros = False)
        dB(v) = max(10 log10(|v| + eps_f32), -200)                              (utils.py:16-40: floor at about -69.2 dB)
        error_db[r][k] = mean_t |dB(E^x_k[r][t]) - dB(E^y_k[r][t])|,  rmse[k] = ||error_db[:, k]||_2 / sqrt(R)  (:656-661)

    The analysis filterbank is a DECLARED INPUT (the reference's comes from pyfar / slope2noise): ``analysis_taps`` (A, Ma)
    causal FIRs, default ``taps``; a band signal is the first L samples of the causal convolution.  The filter is linear, so
    a_k * y[r] = a_k * D[r] + sum_s W[r][s] (a_k * C_s): ``dataset.direct_band_render`` and ``dataset.edc_error_target`` are
    constants (built on the first call, cached; 2.25 GB EACH at 838 receivers x 7 bands x 96 000 samples), the model
    contributes A x bands x G signals (``bank.analysis_group_signals``), and csrc/edcerr.hip composes, squares, scans and
    compares every (receiver, band) without storing the estimate's band signals.  More than 32 group signals: the band
    signals are rendered with ``hip_ops.render_mix`` into a temporary, 128 receivers at a time.

    ``measured`` (R, Tx): tensor or numpy; pass a float32 device tensor for a steady state without host syncs (anything
    else is uploaded and compared by value against the cached target's source).  ``sample_rate`` defaults to the bank's;
    ``rows``: receivers to score, in this order (default all R) -- a job that spreads receivers over ranks passes every rank
    its share, and the job's rmse is the root of the ranks' summed squares over the total count.  Not covered:
    ``norm_edc=True``, position re-ordering, the plots.  The EDR variant (``plot_edr_error_in_space``) is
    ``edr_error_bank``.
    Returns (error_db (len(rows) or R, A), rmse (A,)) float32 on the bank's device."""
    dev = bank.input_gains.device
    taps, at = _edc_taps(bank, taps, analysis_taps)
    if taps.dim() != 2 or taps.shape[0] != bank.num_bands or dataset.num_bands != bank.num_bands or at.dim() != 2:
        raise ValueError("edc_error_bank: one row of taps and one dataset per band of the bank; analysis_taps (A, Ma)")
    fs = float(bank.sample_rate if sample_rate is None else sample_rate)
    R = dataset.R
    if measured.ndim != 2 or measured.shape[0] != R:
        raise ValueError("edc_error_bank: measured (R, Tx), one row per receiver of the dataset")
    Ty = 2 * (dataset.z_values.shape[-1] - 1) + taps.shape[1] - 1
    L = min(int(measured.shape[1]), Ty, int(2 * fs))
    if L < 1:
        raise ValueError("edc_error_bank: no samples to compare")
    sel = _edc_rows(rows, R, dev, "edc_error_bank")
    Dk = dataset.direct_band_render(taps, at, L)
    Tdb = dataset.edc_error_target(measured, at, L)
    W = bank.render_gains(dataset.norm_listener_position, R, sel)
    if W.shape[1] <= 32:
        Ck = bank.analysis_group_signals(dataset.z_values, taps, at, L)
        err = ops.edc_error(Dk, Tdb, L, W=W, Ck=Ck, rows=sel, rows_checked=True)
    else:
        C = bank.filtered_group_signals(dataset.z_values, taps)
        Ck = band_split(C, at, L)                                              # (S, A, L)
        n, A = W.shape[0], at.shape[0]
        err = torch.empty((n, A), dtype=torch.float32, device=dev)
        for i0 in range(0, n, 128):
            i1 = min(i0 + 128, n)
            part = torch.arange(i0, i1, device=dev) if sel is None else sel[i0:i1]
            Y = ops.empty_bands(i1 - i0, A, L, dev)
            for k in range(A):
                ops.render_mix(Dk[:, k], W[i0:i1], Ck[:, k], rows=part, out=Y[:, k])
            ops.edc_error(Y, Tdb.index_select(0, part), L, out=err[i0:i1])
    return err, _rmse(err)


@torch.no_grad()
def edc_error(estimated, measured, analysis_taps, sample_rate: float, rows=None, chunk: int = 32):
    """The metric of ``edc_error_bank`` for ANY rendered RIRs (for instance the output of ``infer_bands``): ``estimated``
    (R, Ty) and ``measured`` (R, Tx), tensors or numpy, ``analysis_taps`` (A, Ma), L = min(Tx, Ty, int(2 sample_rate)).
    Both sides go through ``band_split`` (the estimate's band signals DO pass through memory here: the general path, not
    the bank's) and the same kernel, ``chunk`` receivers at a time.  Returns (error_db (len(rows) or R, A), rmse (A,))."""
    estimated, measured = torch.as_tensor(estimated), torch.as_tensor(measured)
    dev = estimated.device if estimated.is_cuda else measured.device
    if estimated.dim() != 2 or measured.dim() != 2 or estimated.shape[0] != measured.shape[0]:
        raise ValueError("edc_error: estimated (R, Ty) and measured (R, Tx)")
    at = torch.as_tensor(analysis_taps) if not isinstance(analysis_taps, (list, tuple)) else torch.stack(
        [torch.as_tensor(t) for t in analysis_taps])
    at = at.detach().to(device=dev, dtype=torch.float32).contiguous()
    L = min(int(measured.shape[1]), int(estimated.shape[1]), int(2 * float(sample_rate)))
    if L < 1 or at.dim() != 2:
        raise ValueError("edc_error: no samples to compare, or analysis_taps not (A, Ma)")
    R = estimated.shape[0]
    sel = _edc_rows(rows, R, torch.device('cpu'), "edc_error")
    n = R if sel is None else sel.numel()
    err = torch.empty((n, at.shape[0]), dtype=torch.float32, device=dev)
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        part = slice(i0, i1) if sel is None else sel[i0:i1].to(estimated.device)
        y = estimated[part][:, :L].to(device=dev, dtype=torch.float32)
        part = part if sel is None else part.to(measured.device)
        x = measured[part][:, :L].to(device=dev, dtype=torch.float32)
        Tdb = ops.edc_curve_db(band_split(x, at, L), L)
        ops.edc_error(band_split(y, at, L), Tdb, L, out=err[i0:i1])
    return err, _rmse(err)


def _edr_frames(L: int, win_size, hop_size, what: str):
    """(win, T) of the reference's STFT of an L-sample signal (losses.py:501-553); ValueError where it has none"""
    win = int(win_size)
    if hop_size is not None and int(hop_size) != win // 2:
        raise ValueError(f"{what}: hop_size must be win_size // 2 (the reference asserts it, losses.py:524)")
    if win < 4 or win & (win - 1):
        raise ValueError(f"{what}: win_size must be a power of two")
    hop = win // 2
    padded = -(-L // hop) * hop
    if L < 1 or padded < win:
        raise ValueError(f"{what}: {L} samples padded to whole hops are shorter than one window of {win}: no frame")
    return win, (padded - win) // hop + 1


@torch.no_grad()
def edr_error_bank(bank, dataset, taps, measured, win_size: int = 4096, hop_size: Optional[int] = None, rows=None):
    """The EDR matching error of a trained band bank over the receiver grid in one pass: the reference's
    ``plot_edr_error_in_space`` -> ``get_edr_error`` (plot.py:760-874, the metric at :782-822; its "RMSE in matching EDR is
    ... dB" line) of the bank's full-band render (``infer_bank``) against the measured RIRs.

        L = min(Tx, Ty)                                  (plot.py:848-852; no 2 fs clamp here, unlike the EDC metric)
        S^x[r] = STFT(measured[r][:L]),  S^y[r] = STFT(y[r][:L])       (losses.py:501-553 ``get_stft_torch``: zero-padded to
                 whole hops, periodic Hann of win_size, hop = win_size / 2, nfft = win_size, center=False, one-sided)
        EDR[r][f][m] = dB(sum_{tau >= m} |S[r][f][tau]|^2),  dB(v) = max(10 log10(|v| + eps_f32), -200)
                                                      (losses.py:556-575, utils.py:16-40: floor at about -69.2 dB)
        error_db[r] = mean_{f, m} |EDR^x[r] - EDR^y[r]|,  rmse = ||error_db||_2 / sqrt(R)                (plot.py:818-821)

    The STFT is linear, as are truncation and zero padding, so STFT(y[r][:L]) = STFT(D[r][:L]) + sum_s W[r][s] STFT(C_s[:L]):
    ``dataset.direct_render_stft`` and ``dataset.edr_error_target`` are constants (built on the first call, cached; 0.43 GB
    and 0.21 GB at 838 receivers, win 4096 and 64 000 samples, about twice that at 131 200), the model contributes bands x G
    short-time spectra (``bank.stft_group_signals``), and csrc/edrerr.hip composes, squares, sums the tails and compares
    every receiver without storing the estimate's spectra.  More than 32 group signals: the spectra are mixed with
    ``hip_ops.render_mix`` on the float view of the complex rows into a temporary, 128 receivers at a time.

    ``measured`` (R, Tx): tensor or numpy; pass a float32 device tensor for a steady state without host syncs (anything
    else is uploaded and compared by value against the cached target's source).  ``hop_size``: None or win_size // 2 (the
    reference asserts it).  ``rows``: receivers to score, in this order (default all R) -- a job that spreads receivers over
    ranks passes every rank its share.  Not covered: position re-ordering (``order_position_matrices``: rows are the
    dataset's receiver order), the plots, several sources, ERB grouping, and a job-level reduction of ``rmse`` over ranks
    (the root of the ranks' summed squares over the total count).
    Returns (error_db (len(rows) or R,), rmse ()) float32 on the bank's device."""
    dev = bank.input_gains.device
    taps, _ = _edc_taps(bank, taps, None)
    if taps.dim() != 2 or taps.shape[0] != bank.num_bands or dataset.num_bands != bank.num_bands:
        raise ValueError("edr_error_bank: one row of taps and one dataset per band of the bank")
    R = dataset.R
    if measured.ndim != 2 or measured.shape[0] != R:
        raise ValueError("edr_error_bank: measured (R, Tx), one row per receiver of the dataset")
    Ty = 2 * (dataset.z_values.shape[-1] - 1) + taps.shape[1] - 1
    L = min(int(measured.shape[1]), Ty)
    win, T = _edr_frames(L, win_size, hop_size, "edr_error_bank")
    sel = _edc_rows(rows, R, dev, "edr_error_bank")
    Sd = dataset.direct_render_stft(taps, L, win)
    Tdb = dataset.edr_error_target(measured, L, win)
    W = bank.render_gains(dataset.norm_listener_position, R, sel)
    Sc = bank.stft_group_signals(dataset.z_values, taps, L, win)
    if W.shape[1] <= 32:
        err = ops.edr_error(Sd, Tdb, W=W, Sc=Sc, rows=sel, rows_checked=True)
    else:
        n, F = W.shape[0], win // 2 + 1
        err = torch.empty((n,), dtype=torch.float32, device=dev)
        # (the frame rows of both stores have ops.empty_spectra's pitch: a receiver's spectrum is one float32 row)
        d_flat = torch.view_as_real(Sd.as_strided((R, T * Sd.stride(1)), (Sd.stride(0), 1))).flatten(1)
        c_flat = torch.view_as_real(Sc.as_strided((Sc.shape[0], T * Sc.stride(1)), (Sc.stride(0), 1))).flatten(1)
        for i0 in range(0, n, 128):
            i1 = min(i0 + 128, n)
            part = torch.arange(i0, i1, device=dev) if sel is None else sel[i0:i1]
            Y = ops.empty_spectra(i1 - i0, T, F, dev)
            y_flat = torch.view_as_real(Y.as_strided((i1 - i0, T * Y.stride(1)), (Y.stride(0), 1))).flatten(1)
            ops.render_mix(d_flat, W[i0:i1], c_flat, rows=part, out=y_flat)
            ops.edr_error(Y, Tdb.index_select(0, part), out=err[i0:i1])
    return err, _rmse(err)


@torch.no_grad()
def edr_error(estimated, measured, win_size: int = 4096, rows=None, chunk: int = 32):
    """The metric of ``edr_error_bank`` for ANY rendered RIRs (for instance the output of ``infer_bands``): ``estimated``
    (R, Ty) and ``measured`` (R, Tx), tensors or numpy, L = min(Tx, Ty), hop = win_size // 2.  Both sides go through
    ``hip_ops.stft_spectrum`` (the estimate's spectra DO pass through memory here: the general path, not the bank's) and
    the same kernel with no group signals, ``chunk`` receivers at a time.  Returns (error_db (len(rows) or R,), rmse ())."""
    estimated, measured = torch.as_tensor(estimated), torch.as_tensor(measured)
    dev = estimated.device if estimated.is_cuda else measured.device
    if estimated.dim() != 2 or measured.dim() != 2 or estimated.shape[0] != measured.shape[0]:
        raise ValueError("edr_error: estimated (R, Ty) and measured (R, Tx)")
    L = min(int(measured.shape[1]), int(estimated.shape[1]))
    win, _ = _edr_frames(L, win_size, None, "edr_error")
    R = estimated.shape[0]
    sel = _edc_rows(rows, R, torch.device('cpu'), "edr_error")
    n = R if sel is None else sel.numel()
    err = torch.empty((n,), dtype=torch.float32, device=dev)
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        part = slice(i0, i1) if sel is None else sel[i0:i1].to(estimated.device)
        y = estimated[part][:, :L].to(device=dev, dtype=torch.float32).contiguous()
        part = part if sel is None else part.to(measured.device)
        x = measured[part][:, :L].to(device=dev, dtype=torch.float32).contiguous()
        Tdb = ops.edr_curve_db(ops.stft_spectrum(x, L, win))
        ops.edr_error(ops.stft_spectrum(y, L, win), Tdb, out=err[i0:i1])
    return err, _rmse(err)


def _moving_plan(P: int, Lr: int, fs: float, update_ms: float, alpha: float, fade_len_ms: float, what: str):
    """(h, Fd, n) of the reference's moving-listener render; ValueError outside the declared scope"""
    h, Fd = int(update_ms * 1e-3 * fs), int(fade_len_ms * 1e-3 * fs)        # utils.py:62-80 ``ms_to_samps``: truncation
    if P < 1:
        raise ValueError(f"{what}: an empty path")
    if h < 1:
        raise ValueError(f"{what}: update_ms is shorter than one sample")
    if not 1 <= Fd <= h:
        raise ValueError(f"{what}: the cross-fade must be 1 .. {h} samples (one update interval) long, not {Fd}: at 0 the "
                         "reference raises, above one interval it fades with stale samples")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"{what}: 0 <= alpha <= 1")
    if P * h >= 2 ** 31:
        raise ValueError(f"{what}: P h < 2^31 samples")
    return h, Fd, max(16, 1 << (h + Lr - 2).bit_length())


def _moving_stimulus(stimulus, total: int, dev, what: str) -> torch.Tensor:
    """sound_examples.py:149-161 ``create_extended_stimulus``: float32, repeated or cut to ``total`` samples"""
    x = torch.as_tensor(stimulus).detach().to(device=dev, dtype=torch.float32).reshape(-1)
    if x.numel() == 0:
        raise ValueError(f"{what}: an empty stimulus")
    return x.repeat(-(-total // x.numel()))[:total].contiguous()


def _moving_out(out, total: int, dev, what: str) -> torch.Tensor:
    if out is None:
        return torch.zeros((total,), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or tuple(out.shape) != (total,) or not out.is_contiguous() or out.device != torch.device(dev):
        raise ValueError(f"{what}: out must be a contiguous float32 ({total},) vector on the device")
    return out.zero_()


def _moving_run(x, P: int, h: int, Fd: int, Lr: int, n: int, alpha: float, chunk: int, out, chunk_inputs):
    """compose -> inverse transform -> overlap-add, ``chunk`` segments at a time.  ``chunk_inputs(k0, k1)`` returns
    moving_compose's (Dh, rows, W, Ch) for the segments k0 .. k1 - 1."""
    dev = x.device
    blocks = x.view(P, h)
    ema = torch.empty((n // 2 + 1,), dtype=torch.complex64, device=dev)
    tails = [torch.empty((Fd,), dtype=torch.float32, device=dev) for _ in range(2)]
    for i, k0 in enumerate(range(0, P, chunk)):
        k1 = min(k0 + chunk, P)
        Dh, rows, W, Ch = chunk_inputs(k0, k1)
        Z = ops.moving_compose(Dh, ops.rfft_pow2(blocks[k0:k1], n), ema, alpha, k0 == 0, W=W, Ch=Ch, rows=rows,
                               rows_checked=True)
        ops.moving_ola(ops.irfft_pow2_fwd(Z, n), k0, P, h, Lr, Fd, out, tails[i & 1] if k0 else None, tails[1 - (i & 1)])
    return out


@torch.no_grad()
def render_moving_listener_bank(bank, dataset, taps, path, stimulus, update_ms: float = 100.0, alpha: float = 0.5,
                                fade_len_ms: float = 50.0, sample_rate: Optional[float] = None, chunk: int = 32,
                                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A dry stimulus heard by a listener who moves over the receiver grid of a trained band bank, in one pass: the
    reference's ``dynamic_rendering_moving_receiver.filter_overlap_add`` (sound_examples.py:163-226, ``use_whole_rir=True``)
    on the bank's full-band render (``infer_bank``) of the dataset rows ``path``, one row per update interval.

        h = int(update_ms 1e-3 fs),  Fd = int(fade_len_ms 1e-3 fs),  total = P h                   (utils.py:62-80; :102, :169)
        x = the stimulus as float32, repeated or cut to total samples,  x_k = x[k h : (k + 1) h]             (:149-161, :195)
        f_0 = r_0,  f_k = alpha r_k + (1 - alpha) f_{k-1},  r_k = y[path[k]]   (:184-193: the recursion runs on the FILTER)
        s_k = fftconvolve(x_k, f_k, 'full')[: min(h + Lr - 1, total - k h)]                                      (:196-203)
        out[k h + i] += s_k[i];  for k >= 1 and i < Fd instead  t_{k-1}[i] fade_out[i] + s_k[i] fade_in[i]       (:205-217)
        fade_in = 0.5 (1 + linspace(-1, 1, Fd)),  fade_out = 1 - fade_in,  t_{k-1} = the LAST Fd samples of s_{k-1}
                                                                                                       (:118-127, :219-224)

    Transform, interpolation and the bank's composition are linear, so with n the power of two >= h + Lr - 1 the spectrum of
    f_k is the running average of Dh[path[k]] + sum_s W[k][s] Ch[s]: ``dataset.direct_render_spectrum(taps, n)`` is a
    constant (built on the first call, cached; 0.88 GB at 838 receivers and n = 2^18), the model contributes bands x G
    spectra (``rfft_pow2(bank.filtered_group_signals(...), n)``) and the gains ``bank.render_gains(..., path)``, and
    csrc/moving.hip composes, interpolates and multiplies per bin, then overlap-adds the inverse transforms
    (``irfft_pow2_fwd``), ``chunk`` segments at a time: neither the composed RIRs nor the interpolated filters are stored.
    More than 32 group signals: the rows are rendered with ``infer_bank(rows=path)`` and go through
    ``render_moving_listener``.

    ``path``: P dataset rows, repeats and any order allowed; ``stimulus``: 1-D, tensor or numpy; ``sample_rate`` defaults
    to the bank's; ``out``: a contiguous float32 (P h,) buffer to fill.  Scope: P >= 1, h >= 1 and 1 <= Fd <= h (at Fd = 0
    the reference raises, above h its tail buffer keeps stale samples: ValueError here), 0 <= alpha <= 1.  Every call
    starts fresh: the ``prev_filter`` that the reference leaves on its object between calls is not reproduced.  Not covered:
    the late-RIR variant (pass late RIRs to ``render_moving_listener``), loudness normalisation, the animation, wav
    export.  Binaural / HRTF rendering of the directional model is ``render_binaural_moving_listener_bands`` and
    ``render_binaural_moving_listener``.
    Returns (P h,) float32 on the bank's device."""
    what = "render_moving_listener_bank"
    dev = bank.input_gains.device
    taps, _ = _edc_taps(bank, taps, None)
    if taps.dim() != 2 or taps.shape[0] != bank.num_bands or dataset.num_bands != bank.num_bands:
        raise ValueError(f"{what}: one row of taps and one dataset per band of the bank")
    if path is None or torch.as_tensor(path).numel() == 0:
        raise ValueError(f"{what}: an empty path")
    sel = _edc_rows(path, dataset.R, dev, what)
    P = sel.numel()
    fs = float(bank.sample_rate if sample_rate is None else sample_rate)
    Lr = 2 * (dataset.z_values.shape[-1] - 1) + taps.shape[1] - 1
    h, Fd, n = _moving_plan(P, Lr, fs, update_ms, alpha, fade_len_ms, what)
    if bank.num_bands * bank.num_groups > 32:
        y = infer_bank(bank, dataset, taps, rows=sel)
        return render_moving_listener(y, None, stimulus, fs, update_ms, alpha, fade_len_ms, chunk, out)
    x = _moving_stimulus(stimulus, P * h, dev, what)
    out = _moving_out(out, P * h, dev, what)
    Dh = dataset.direct_render_spectrum(taps, n)
    W = bank.render_gains(dataset.norm_listener_position, dataset.R, sel)
    Ch = ops.rfft_pow2(bank.filtered_group_signals(dataset.z_values, taps), n)
    return _moving_run(x, P, h, Fd, Lr, n, float(alpha), int(chunk), out,
                       lambda k0, k1: (Dh, sel[k0:k1], W[k0:k1], Ch))


@torch.no_grad()
def render_moving_listener(rirs, path, stimulus, fs: float, update_ms: float = 100.0, alpha: float = 0.5,
                           fade_len_ms: float = 50.0, chunk: int = 32, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The render of ``render_moving_listener_bank`` for ANY RIR matrix (for instance the output of ``infer_bands``, or the
    late RIRs of a dataset: the reference's ``use_whole_rir=False``): ``rirs`` (R, Lr) tensor or numpy, ``path``: P of its
    rows (None: every row in order), ``stimulus`` 1-D, ``fs`` the sample rate.  The rows' spectra DO pass through memory
    here, ``chunk`` segments at a time (the general path, not the bank's), into the same kernels with no group signals.
    Returns (P h,) float32 on the device of ``rirs`` (a host matrix: on the current device)."""
    what = "render_moving_listener"
    rirs = torch.as_tensor(rirs)
    if rirs.dim() != 2 or rirs.shape[1] < 1:
        raise ValueError(f"{what}: rirs (R, Lr)")
    dev = rirs.device if rirs.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if path is None:
        sel = torch.arange(rirs.shape[0])
    else:
        if torch.as_tensor(path).numel() == 0:
            raise ValueError(f"{what}: an empty path")
        sel = _edc_rows(path, rirs.shape[0], torch.device("cpu"), what)
    sel = sel.to(rirs.device)
    P, Lr = sel.numel(), int(rirs.shape[1])
    h, Fd, n = _moving_plan(P, Lr, float(fs), update_ms, alpha, fade_len_ms, what)
    x = _moving_stimulus(stimulus, P * h, dev, what)
    out = _moving_out(out, P * h, dev, what)

    def chunk_inputs(k0, k1):
        r = rirs[sel[k0:k1]].to(device=dev, dtype=torch.float32)
        return ops.rfft_pow2(r, n), None, None, None
    return _moving_run(x, P, h, Fd, Lr, n, float(alpha), int(chunk), out, chunk_inputs)


def _binaural_plan(P: int, L: int, fs: float, update_ms: float, alpha: float, fade_len_ms, rotations, hrir_sh, Ls: int,
                   dev, what: str):
    """(h, Fd, nb, n2, rot (P, Ls, Ls), Hh (Ls, 2, nb / 2 + 1)) of the reference's binaural render; ValueError outside the
    declared scope"""
    fade_len_ms = update_ms if fade_len_ms is None else fade_len_ms         # sound_examples.py:478
    if L < 9:
        raise ValueError(f"{what}: ambisonic RIRs of at least 9 samples (the transforms start at 16 points)")
    nb = 1 << (L - 1).bit_length()                                          # :408, 2^ceil(log2 L)
    h, Fd, n2 = _moving_plan(P, nb, fs, update_ms, alpha, fade_len_ms, what)
    rot = torch.as_tensor(rotations).detach().to(device=dev, dtype=torch.float32)
    if tuple(rot.shape) != (P, Ls, Ls):
        raise ValueError(f"{what}: rotations must be ({P}, {Ls}, {Ls}): one real SH rotation matrix per path position")
    hr = torch.as_tensor(hrir_sh).detach().to(device=dev, dtype=torch.float32)
    if hr.dim() != 3 or hr.shape[0] != Ls or hr.shape[1] != 2 or hr.shape[2] < 1:
        raise ValueError(f"{what}: hrir_sh must be ({Ls}, 2, Mh): the SH-domain HRIRs of both ears")
    if hr.shape[2] > nb:
        raise ValueError(f"{what}: HRIRs of {hr.shape[2]} samples are longer than the transform of {nb}: the reference "
                         "would silently truncate them")
    Hh = ops.rfft_pow2(hr.reshape(Ls * 2, -1).contiguous(), nb).view(Ls, 2, nb // 2 + 1)
    return h, Fd, nb, n2, rot.contiguous(), Hh


def _binaural_out(out, total: int, dev, what: str) -> torch.Tensor:
    if out is None:
        return torch.zeros((total, 2), dtype=torch.float32, device=dev)
    if (out.dtype != torch.float32 or tuple(out.shape) != (total, 2) or not out.is_contiguous()
            or out.device != torch.device(dev)):
        raise ValueError(f"{what}: out must be a contiguous float32 ({total}, 2) matrix on the device")
    return out.zero_()


def binaural_compose_torch(rot, Hh, alpha: float, k0: int, nseg: int, Ah, row_off: int = 0) -> torch.Tensor:
    """``hip_ops.binaural_compose`` in rows mode in stock tensor operations, the reference's order of operations
    (interpolate, rotate, contract with the conjugated HRTFs): for more than 16 channels, and the float32 yardstick of the
    kernel's bound in tests/test_gpu_binaural.py."""
    k = torch.arange(k0, k0 + nseg, device=rot.device)
    kp = (k - 1).clamp_(min=0)
    a = torch.where(k == 0, 1.0, float(alpha)).to(torch.float32)
    Rw = a.view(-1, 1, 1) * rot[k] + (1.0 - a).view(-1, 1, 1) * rot[kp]
    Aw = a.view(-1, 1, 1) * Ah[k - row_off] + (1.0 - a).view(-1, 1, 1) * Ah[kp - row_off]
    rotated = torch.matmul(Rw.to(Aw.dtype), Aw)                                      # (nseg, Ls, Kb)
    return torch.einsum('nef,knf->kef', Hh.conj(), rotated)


def _binaural_run(x, P: int, h: int, Fd: int, nb: int, n2: int, chunk: int, out, compose):
    """compose -> BRIRs at nb -> their spectra at n2 -> product with the stimulus blocks' -> inverse transform ->
    overlap-add, ``chunk`` segments at a time.  ``compose(k0, k1)`` returns B (k1 - k0, 2, nb / 2 + 1)."""
    dev = x.device
    blocks = x.view(P, h)
    tails = [torch.empty((Fd, 2), dtype=torch.float32, device=dev) for _ in range(2)]
    for i, k0 in enumerate(range(0, P, chunk)):
        k1 = min(k0 + chunk, P)
        B = compose(k0, k1)
        brir = ops.irfft_pow2_fwd(B.reshape(-1, B.shape[-1]), nb)                    # circular at nb, as the reference's
        Z = ops.rfft_pow2(brir, n2).view(k1 - k0, 2, -1) * ops.rfft_pow2(blocks[k0:k1], n2).unsqueeze(1)
        s = ops.irfft_pow2_fwd(Z.view(2 * (k1 - k0), -1), n2).view(k1 - k0, 2, n2)
        ops.binaural_ola(s, k0, P, h, nb, Fd, out, tails[i & 1] if k0 else None, tails[1 - (i & 1)])
    return out


@torch.no_grad()
def render_binaural_moving_listener_bands(nets, z_values, norm_listener_position, taps, length: int, hrir_sh, path,
                                          rotations, stimulus, update_ms: float = 100.0, alpha: float = 0.5,
                                          fade_len_ms: Optional[float] = None, sample_rate: Optional[float] = None,
                                          chunk: int = 32, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A dry stimulus heard over headphones by a listener who walks over the receiver grid and turns their head, from the
    trained directional bands in one pass: the reference's ``binaural_dynamic_rendering.binaural_filter_overlap_add``
    (sound_examples.py:356-535) on the ambisonic RIRs ``infer_directional_bands(.., directional=False, rows=path)``, one
    row and one head orientation per update interval.  With Ls = (order + 1)^2, L the RIRs' length:

        nb = 2^ceil(log2 L),  Kb = nb / 2 + 1;   A_k = rfft(a[path[k]], nb),  Hh = rfft(hrir_sh, nb)              (:408-422)
        h = int(update_ms 1e-3 fs),  Fd = int(fade_len_ms 1e-3 fs) (default: = h),  total = P h          (utils.py:62-80; :478)
        x = the stimulus as float32, repeated or cut to total;  x_k = x[k h : (k + 1) h]                          (:149-161)
        Rw_0 = R_0,  Rw_k = alpha R_k + (1 - alpha) R_{k-1};   Aw_0 = A_0,  Aw_k = alpha A_k + (1 - alpha) A_{k-1}  (:450-461)
        B_k[e][f] = sum_n conj(Hh[n][e][f]) sum_m Rw_k[n][m] Aw_k[m][f];   b_k[e] = irfft(B_k[e], nb)             (:463-469)
        s_k[e] = fftconvolve(x_k, b_k[e], 'full')[: min(h + nb - 1, total - k h)]                                 (:503-511)
        out[k h + i][e] += s_k[e][i];  for k >= 1 and i < Fd instead  t_{k-1}[e][i] fade_out[i] + s_k[e][i] fade_in[i]
        fade_in = sqrt(0.5 (1 + linspace(-1, 1, Fd))),  fade_out = sqrt(0.5 (1 - linspace(-1, 1, Fd))),
        t_{k-1}[e] = the LAST Fd samples of the cut s_{k-1}[e]                                    (:118-127, :480-485, :527-533)

    The reference's quirks are kept: NO recursion -- the interpolation takes the RAW previous position and orientation
    (the omnidirectional ``render_moving_listener_bank`` recurses on the filter); the HRTFs enter CONJUGATED and the BRIR is
    a CIRCULAR product at nb; the reference indexes its RIR store by the segment number, its dataset being the path in
    order: here ``path`` selects the rows, a_k = a[path[k]].  The receiver enters the directional render only through its
    SH weights, so with C the Q G Ls band signals and W the weights of ``infer_directional_bands``

        B_k[e][f] = sum_n conj(Hh[n][e][f]) sum_m Rw_k[n][m] sum_s Wk_k[s][m] rfft(C, nb)[s Ls + m][f]

    (csrc/binaural.hip): the path's ambisonic RIRs and their spectra never exist.  The BRIRs are the exception: circular at
    nb, convolved at n2 = the power of two >= h + nb - 1, a chunk's BRIRs (chunk x 2 x nb floats) pass through memory once
    between the two transforms.  The product with the stimulus blocks' spectra is stock complex multiplication.

    ``nets``, ``z_values``, ``norm_listener_position``, ``taps``, ``length``: as ``infer_directional_bands``.  ``hrir_sh``
    (Ls, 2, Mh): the HRIRs in the SH domain, a DECLARED INPUT (the reference reads a SOFA file and calls
    ``get_spherical_harmonic_representation(order)``); Mh <= nb, a longer set is a ValueError (the reference would silently
    truncate it).  ``rotations`` (P, Ls, Ls): the real SH rotation matrices, a DECLARED INPUT -- the convention is the
    reference's call ``spaudiopy.sph.sh_rotation_matrix(order, -yaw, +el, 0, 'real')`` per position, after its own sign
    flip of the elevation (:388, :444-449).  ``path``: P rows of ``norm_listener_position``, repeats and any order allowed;
    ``stimulus``: 1-D, tensor or numpy; ``sample_rate`` defaults to the nets'; ``out``: a contiguous float32 (P h, 2) buffer.
    Scope: P >= 1, h >= 1, 1 <= Fd <= h, 0 <= alpha <= 1, P h < 2^31, L >= 9.  Every call starts fresh: the ``prev_*`` state
    that the reference leaves on its object is not reproduced; the reference's constructor always takes ``late_rirs``, here
    the RIRs are the bands' (pass others to ``render_binaural_moving_listener``).  More than 32 band signals per channel
    or 16 channels: the rows are rendered with ``infer_directional_bands`` and go through
    ``render_binaural_moving_listener``.  Not covered: a SOFA reader, building rotation matrices from angles, loudness
    normalisation, the animation, wav export.
    Returns (P h, 2) float32, ears interleaved as the reference returns them."""
    what = "render_binaural_moving_listener_bands"
    nets = list(nets)
    if path is None or torch.as_tensor(path).numel() == 0:
        raise ValueError(f"{what}: an empty path")
    if not nets:
        raise ValueError(f"{what}: no bands")
    fs = float(getattr(nets[0], "sample_rate") if sample_rate is None else sample_rate)
    G, Ls = nets[0].num_groups, nets[0].num_delay_lines_per_group
    if len(nets) * G > ops.BINAURAL_MAX_S or Ls > ops.BINAURAL_MAX_LS:
        y = infer_directional_bands(nets, z_values, norm_listener_position, taps, length, directional=False, rows=path)
        return render_binaural_moving_listener(y, hrir_sh, None, rotations, stimulus, fs, update_ms, alpha, fade_len_ms,
                                               chunk, out)
    dev = nets[0].output_gains.device
    P = torch.as_tensor(path).numel()
    L = max(1, min(int(length), 2 * (z_values.shape[-1] - 1)))
    h, Fd, nb, n2, rot, Hh = _binaural_plan(P, L, fs, update_ms, alpha, fade_len_ms, rotations, hrir_sh, Ls, dev, what)
    x = _moving_stimulus(stimulus, P * h, dev, what)
    W, C, _, _ = _directional_inputs(nets, z_values, norm_listener_position, taps, length, path, 4096, what)
    out = _binaural_out(out, P * h, dev, what)
    Ch = ops.rfft_pow2(C, nb)
    return _binaural_run(x, P, h, Fd, nb, n2, int(chunk), out,
                         lambda k0, k1: ops.binaural_compose(rot, Hh, float(alpha), k0, k1 - k0, W=W, Ch=Ch))


@torch.no_grad()
def render_binaural_moving_listener(ambi_rirs, hrir_sh, path, rotations, stimulus, fs: float, update_ms: float = 100.0,
                                    alpha: float = 0.5, fade_len_ms: Optional[float] = None, chunk: int = 32,
                                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The render of ``render_binaural_moving_listener_bands`` for ANY ambisonic RIRs (for instance a measured dataset's, or
    its late parts, which the reference's constructor always takes): ``ambi_rirs`` (R, Ls, L) tensor or numpy, ``path``: P
    of its rows (None: every row in order), ``hrir_sh`` (Ls, 2, Mh), ``rotations`` (P, Ls, Ls), ``stimulus`` 1-D, ``fs`` the
    sample rate.  The rows' spectra DO pass through memory here, ``chunk`` segments at a time (the general path, not the
    bands'), into the same kernels in rows mode; more than 16 channels: the composition in stock tensor operations
    (``binaural_compose_torch``).  The same quirks and scope.
    Returns (P h, 2) float32 on the device of ``ambi_rirs`` (a host array: on the current device)."""
    what = "render_binaural_moving_listener"
    rirs = torch.as_tensor(ambi_rirs)
    if rirs.dim() != 3 or rirs.shape[1] < 1 or rirs.shape[2] < 1:
        raise ValueError(f"{what}: ambi_rirs (R, Ls, L)")
    dev = rirs.device if rirs.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if path is None:
        sel = torch.arange(rirs.shape[0])
        if sel.numel() == 0:
            raise ValueError(f"{what}: an empty path")
    else:
        if torch.as_tensor(path).numel() == 0:
            raise ValueError(f"{what}: an empty path")
        sel = _edc_rows(path, rirs.shape[0], torch.device("cpu"), what)
    sel = sel.to(rirs.device)
    P, Ls, L = sel.numel(), int(rirs.shape[1]), int(rirs.shape[2])
    h, Fd, nb, n2, rot, Hh = _binaural_plan(P, L, float(fs), update_ms, alpha, fade_len_ms, rotations, hrir_sh, Ls, dev, what)
    x = _moving_stimulus(stimulus, P * h, dev, what)
    out = _binaural_out(out, P * h, dev, what)

    def compose(k0, k1):
        lo = max(k0 - 1, 0)                                                          # (the raw previous position)
        r = rirs[sel[lo:k1]].to(device=dev, dtype=torch.float32).reshape(-1, L)
        Ah = ops.rfft_pow2(r, nb).view(k1 - lo, Ls, -1)
        if Ls > ops.BINAURAL_MAX_LS:
            return binaural_compose_torch(rot, Hh, float(alpha), k0, k1 - k0, Ah, lo).contiguous()
        return ops.binaural_compose(rot, Hh, float(alpha), k0, k1 - k0, Ah=Ah, row_off=lo)
    return _binaural_run(x, P, h, Fd, nb, n2, int(chunk), out, compose)


def sum_bands(local_band_rirs: Sequence[torch.Tensor], group=None, dst: int = 0, device=None) -> Optional[torch.Tensor]:
    """Sum of the filtered RIRs over ALL bands (reference :358 ``groupby('position').apply(sum)``):
    local sum over this rank's bands, then one reduce to ``dst``.  Returns the total on ``dst``,
    None elsewhere.  A rank WITHOUT bands (8 ranks, 7 bands) passes []: the shape, dtype of the result are agreed
    on first (an all-reduce MAX of a 3-word header) and the rank contributes zeros; ``device`` is where it builds
    them (default: the current CUDA device, or the CPU when there is none)."""
    local = list(local_band_rirs)
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1:
        if not local:
            raise ValueError("sum_bands: no bands")
        return torch.stack(local, dim=0).sum(dim=0)
    if local:
        total = torch.stack(local, dim=0).sum(dim=0)
        if total.dim() != 2:
            raise ValueError("sum_bands: (receivers, samples) tensors expected")
        device = total.device
    else:
        total = None
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
    dtypes = [torch.float32, torch.float64]
    head = torch.tensor([0, 0, 0] if total is None else [total.shape[0], total.shape[1], dtypes.index(total.dtype)],
                        dtype=torch.int64, device=device)
    dist.all_reduce(head, op=dist.ReduceOp.MAX, group=group)
    shape, dtype = (int(head[0]), int(head[1])), dtypes[int(head[2])]
    if total is None:
        if shape[0] == 0:
            raise ValueError("sum_bands: no rank holds a band")
        total = torch.zeros(shape, dtype=dtype, device=device)
    elif tuple(total.shape) != shape:
        raise ValueError("sum_bands: the ranks' band responses differ in shape")
    dist.reduce(total, dst=dst, op=dist.ReduceOp.SUM, group=group)
    return total if dist.get_rank(group) == dst else None
