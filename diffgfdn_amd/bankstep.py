"""The band bank's optimiser step as an explicit launch sequence (no autograd), on the polynomial form of the
block transfer functions (csrc/blocktf.hip).

What the reference does per batch and band (src/diff_gfdn/trainer.py:373-379, :452-477): ``normalize`` (no-grad
sub-FDN forward, b, c /= E^(1/4)), forward (model.py:569-625), losses (trainer.py:259-315), ``backward()``,
``optimizer.step()``.  With zero coupling and blocks of at most eight delay lines every one of those stages sees the
feedback loop only through the group transfer functions T_g(z) -- ratios of multilinear polynomials in the phasors
z^{m_i} with 2 x 16 (<= 4 lines) or 2 x 256 (5..8 lines, evaluated on the matrix cores) real coefficients per block --
so the step is (the timed form: the linear step with all of round 5's arrangements; DESIGN.md section 5 has the launch
sequence with times, the class attributes below select the older forms for cross-checks)

    main  : group responses T_g filt of the band's G groups from the PERSISTENT records (left by the previous step's tail)
            -> their inverse transform (3 passes; unscaled: normalize's scale sits in the receiver gains) -> their STFT
            -> [gains] EDR loss on spectra composed per receiver as Sd[row] + sum_g gain[b][g] STFT(tau_g), with the sums of
            the gradient spectra over the band's receivers in the same launch -> adjoint STFT -> merge with the EDC part
            -> adjoint transform (3 passes) -> records pass -> tail: parameter gradients -> Adam on M, b, c -> the NEXT
            step's Q, Q Q and record sets (one launch)
    side2 : energy pass (normalize) -> gain network forward -> finish (b, c rescaled, scale, gains x scale) -> mask draw
            -> [group signals] EDC term (one register-resident launch per receiver) -> sum of dL/dx over the band's
            receivers -> colorless pass + sparsity terms -> reported sums -> gain network backward -> its Adam range
            -> next step's receivers

Blocks of 5..8 lines: the same with the coefficient records (csrc/blocktf8.hip) in place of the persistent records, the
forward group responses on the matrix cores and normalize / colorless pass / both adjoints as real transforms of the
coefficient sequences (csrc/polyfft.hip) where the delay lengths are integers on the reference's own grid.

28 launches per step of all bands (4-line blocks); every gradient lands directly in the optimiser's flat gradient buffer (no
accumulate / pack kernels), neither the (K, N) delay-line responses of the per-bin solve nor any per-receiver spectrum or
time signal exists.  The autograd path of ``BandBankTrainer._step_losses`` (per-bin elimination kernels) stays as the
general fallback and as the cross-check of this one (tests/test_gpu_bank.py).
"""
import contextlib
from typing import Dict, NamedTuple, Optional

import torch

from . import hip_ops as ops
from .functional import FrequencyGrid
from .losses import shard_loss_scales


# What ``FusedBankStep._plan`` decides before a step's first launch
_Plan = NamedTuple('_Plan', [
    # sizes: bands, groups, lines per group, bins, bins the transforms read, receivers (all / per band), STFT and EDC windows
    ('nb', int), ('G', int), ('n', int), ('K', int), ('Ku', int), ('Btot', int), ('Bper', int), ('win', int), ('start', int),
    ('length', int),
    # cached tables: slot order, slot of a time sample, (nfft, slot of bin, T) of the transform polynomials, EDC windows
    ('order', Optional[tuple]), ('sot', Optional[torch.Tensor]), ('tfp', Optional[tuple]),
    ('item_len', Optional[torch.Tensor]), ('band_len', Optional[torch.Tensor]),
    # the call
    ('train', bool), ('normalize_first', bool), ('opt_step', bool), ('reduced', bool), ('piped', bool),
    # block regime: 5..8 lines; <= 4 lines with the scale joining late; 5..8 lines with the passes as transforms
    ('big', bool), ('late', bool), ('late8', bool),
    # output stage: time domain; composed spectra; stored signals pair-interleaved / with the folded transform
    ('lin', bool), ('spec', bool), ('pairs', bool), ('fold', bool),
    # the rest: see _plan
    ('gfold', bool), ('parts_in_mlp', bool), ('net_first', bool), ('edc_one', bool), ('late_colorless', bool),
    ('use_tail', bool), ('use_tail8', bool), ('keep_records', bool)])


class _Step:
    """State of one step: its inputs, the streams, the events, the keep list and what earlier stages left for later ones
    (attributes a form does not produce stay None)"""
    scale = Hg = Ts = Dinv8 = ework = Xsub = rgain0 = rgain = xhat = rstd = H = Tq = tau = eye = xd = None
    ev_ts = ev_gam = gH = gsig = gsig_b = g_edc = gam_edr = parts = grg = None

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def on_side2(self):       # (a branch that has no stream of its own runs inline on the main stream)
        return torch.cuda.stream(self.side2) if self.side2 is not None else contextlib.nullcontext()


class FusedBankStep:
    """Explicit forward / backward of ``BandBankTrainer`` for zero-coupling blocks of <= 8 lines and <= 4 groups per band
    (<= 4 lines: csrc/blocktf.hip; 5..8 lines: csrc/blocktf8.hip).  ``supported(trainer)`` tells whether a trainer's
    layout qualifies."""

    @staticmethod
    def supported(trainer) -> bool:
        """Blocks of <= 4 lines: any grid; blocks of 5..8 lines: grids on the unit circle only (``run`` refuses others, and
        the trainer's configuration is the only place that knows before the first batch arrives)."""
        bank = trainer.net
        if bank.coupled:
            return False        # (the records are those of independent blocks: A must be block-diagonal)
        if bank.num_delay_lines_per_group > 4 and getattr(trainer.config, 'reduced_pole_radius', 1.0) != 1.0:
            return False
        return (bank.num_delay_lines_per_group <= 8 and bank.num_groups <= 4
                and bank.num_bands * bank.num_groups <= 64)

    def __init__(self, trainer):
        self.tr = trainer
        bank, opt = trainer.net, trainer.optimizer
        views = {id(p): v for p, v in zip(opt._params, opt._grad_views)}
        # the flat gradient buffer's slices of the four stacked leaves: kernels write them directly
        self.g_c = views[id(bank.output_gains)].view(-1)
        self.g_b = views[id(bank.input_gains)].view(-1)
        self.g_w = views[id(bank.output_scalars_w)].view(-1)
        self.g_M = views[id(bank.feedback_loop_M)].view(bank.num_bands * bank.num_groups,
                                                        bank.num_delay_lines_per_group,
                                                        bank.num_delay_lines_per_group)
        dev = bank.input_gains.device
        nblk = bank.num_bands * bank.num_groups
        self._zero_loss = torch.zeros(nblk, dtype=torch.float32, device=dev)
        self._keep = []
        self._keep_prev = []
        self.w_range = opt.flat_range(bank.output_scalars_w)
        if self.w_range[1] != opt.flat_grad.numel():
            raise RuntimeError("the gain network's parameters must close the flat buffers (BandBankTrainer's group order)")
        self._off = (opt.flat_range(bank.feedback_loop_M)[0], opt.flat_range(bank.input_gains)[0],
                     opt.flat_range(bank.output_gains)[0])
        # Q, QQ and the two record sets of the CURRENT parameters (blocks of <= 4 lines): the fused tail of a training step
        # leaves the next step's here, so that a step does not start with their launch
        self._rec = None
        self._rec_valid = False
        self._rec_versions = None

    # -- records that outlive a step -------------------------------------------------------------------------------------
    def _records(self):
        if self._rec is None:
            bank = self.tr.net
            nblk, n = bank.num_bands * bank.num_groups, bank.num_delay_lines_per_group
            dev = bank.input_gains.device
            mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
            if n > 4:
                # blocks of 5..8 lines: Q, Q Q and the snapshot of the output gains the forward pass reads (the coefficient
                # records themselves are a launch of 500 workgroups at the step's head: csrc/blocktf8.hip)
                self._rec = (mk(nblk, n, n), mk(nblk, n, n), mk(nblk * n))
            else:
                self._rec = (mk(nblk, n, n), mk(nblk, n, n), mk(nblk, 32), mk(nblk, 32))
        return self._rec

    def _versions(self):
        bank = self.tr.net
        leaves = [bank.feedback_loop_M, bank.input_gains, bank.output_gains]
        for net in getattr(bank, 'nets', ()):              # (the bands' own modules hold views of the stacked leaves)
            leaves.extend(p for name, p in net.named_parameters() if 'output_scalars' not in name)
        return tuple(p._version for p in leaves)

    def records_ok(self) -> bool:
        """Whether the kept records belong to the current parameters (host-side bookkeeping: every path of this package that
        changes M, b, c calls :meth:`invalidate_records` or bumps a tensor version)"""
        return self._rec_valid and self._rec_versions == self._versions()

    def invalidate_records(self):
        self._rec_valid = False

    @torch.no_grad()
    def prime_records(self):
        """Records of the current parameters into the kept buffers (one launch on the current stream)"""
        bank = self.tr.net
        if bank.num_delay_lines_per_group > 4:
            Q, QQ, cs = self._records()
            q, qq = ops.ortho_fwd(bank._blocks().detach(), True, True)
            Q.copy_(q)
            QQ.copy_(qq)
            cs.copy_(bank.output_gains.data.view(-1))
            self._rec_valid, self._rec_versions = True, self._versions()
            return
        ops.tf_ortho_coefs(bank._blocks().detach(), bank.inv_gamma, bank.input_gains.data.view(-1),
                           bank.output_gains.data.view(-1), out=self._records())
        self._rec_valid, self._rec_versions = True, self._versions()

    def ensure_records(self):
        """In front of a graph replay whose capture found valid records (and therefore holds no records launch)"""
        if self._rec is not None and not self.records_ok():
            self.prime_records()

    # ---- forms of the step.  Plain class attributes: the defaults are the timed path; tests switch the first six off to check
    # a form against the one it replaced (tests/test_gpu_bank.py, tests/test_gpu_fullsize.py, tests/test_gpu_bankstep_order.py),
    # bench.py reads the last three.  Forms that nothing selects are not kept as switches: they live in git history and
    # NEGATIVES.md, and what was measured and did not pay is described in DESIGN.md section 4.3.
    #
    # The output stage in the TIME domain (csrc/linear.hip): the inverse transform is linear and neither the group transfer
    # functions nor the band's filter depend on the receiver, so x[b] = xd[row_b] + sum_g rgain[b][g] irfft(s_g T_g filt) with
    # xd = irfft(direct filt) a constant of the dataset (BandStackedDataset.direct_time).  A step then runs G forward and G
    # adjoint transforms per band instead of one per receiver (28 instead of 224 at the north-star size), dL/drgain is a
    # dot product over the time samples and the records pass reads G adjoint spectra per band.  Off: the stored-signal chain
    # with the output stage H = (sum_g rgain s_g T_g + direct) filt formed INSIDE the first pass of the forward transform
    # where the sizes allow (gfdn_irfft_odd_pairs_compose_fwd; round 3's path; also what receiver counts outside the linear
    # kernels' limits and chained steps take).
    linear_transforms = True
    # ... and the EDR loss on linearly COMPOSED short-time spectra (csrc/edrlin.hip): the STFT is linear too, so a receiver's
    # spectrum is Sd[row] + sum_g rgain[b][g] STFT(tau_g) with Sd a constant of the dataset (BandStackedDataset.direct_stft).
    # A step runs G forward and G adjoint STFTs per band (the adjoint as ONE launch for all frames, odd frames to a second
    # signal set); per receiver only streaming arithmetic on (frame, frequency) cells is left and the receivers' signals are
    # never stored.  The colorless pass then runs BEHIND the EDC launches, as it does for blocks of 5..8 lines.
    spectral_edr = True
    # The EDC term as ONE register-resident launch per receiver (csrc/edcone.hip: compose, both scans, dB stage, dL/dx and the
    # EDC part of dL/drgain without staging the window samples or dL/dEDC through memory), the EDC part of dL/dtau summed over
    # the band's receivers straight behind it on the side stream; the main chain merges it with the adjoint STFT's two signal
    # sets (three small arrays) into the transform's slot order.  Off, and for windows beyond the launch's 49 152 samples: the
    # three scan launches + one sweep (gfdn_lin_gamma_dots) for the G sums and the EDC part of dL/drgain.
    edc_one_launch = True
    # normalize OFF the critical chain: T is bilinear in b, c and the transform is linear, so the normalisation scale can join
    # the group signals where the forward transform's LAST pass stores them; the energy pass runs on the side stream beside the
    # group responses and the transform's first two passes instead of in front of them (~28 us of chain).  With the
    # wave-per-receiver gain network (ops.mlp_bwd_takes_parts) the scale sits INSIDE the receiver gains: the finish launch of
    # the energy pass stores gain s beside the gains, every launch of the linear step takes those on group signals of the
    # UNSCALED functions, the network's backward multiplies its incoming rows by s and the records pass divides dL/dT by s --
    # the transform's last pass then waits for nothing.
    scale_late = True
    # tail and head as one launch (single process): records -> parameter gradients -> Adam on the blocks' own M, b, c -> the
    # NEXT step's Q, QQ and record sets (csrc/blocktf.hip k_tf_tail, csrc/blocktf8.hip k_tf8_tail); the gain network's range
    # of the flat buffers is stepped on the side stream behind its own backward.  A step then starts with the group responses.
    fused_tail = True
    # blocks of 5..8 lines: the polynomial passes as real transforms of the coefficient sequences (csrc/polyfft.hip) where the
    # delay lengths are integers and the grid is the reference's rfftfreq grid -- ~45 transform-flops per bin and polynomial
    # instead of 512 products; the matrix-core passes (csrc/blocktf8.hip) stay for every other grid
    transform_polys = True
    # the sum of the gradient spectra over the band's receivers inside the EDR launch (k_edr_lin_wave: a thread owns cells of
    # the band's plane and walks the receivers; dL/d|S|^2 never exists, the direct-path spectra are read once), the band's
    # receivers cut into runs for more loads in flight.  Off: the value-only column kernel + the sum as two launches (the
    # cross-check form)
    edr_one_launch = True
    # (0 = two runs: measured same-box, 7 bands: 1 / 2 / 4 runs 0.379 / 0.358 / 0.370 ms; one band: 2 / 4 / 8 / 16 runs 0.222 /
    # 0.227 / 0.229 / 0.229 ms -- every run is one more set of partial planes for the adjoint STFT to add on load)
    edr_receiver_runs = 0

    def _edr_runs(self, nbands: int, B: int) -> int:
        if self.edr_receiver_runs > 0:
            return min(self.edr_receiver_runs, B)
        return 2 if B >= 4 else 1
    # planes stored in the tiled cell order (frequency blocks of 256, a block's frames contiguous): what a (receiver,
    # frequency block) workgroup of the EDR kernel touches is one contiguous run
    tiled_spectra = True

    def _eye_rows(self, nb: int, G: int, device) -> torch.Tensor:
        """(nb * G, G): "receiver" g of every band with gain 1 on group g -- what turns the output-stage kernels into
        H_g = T_g filt and its adjoint (cached: captured graphs hold its pointer)"""
        key = (nb, G, str(device))
        if getattr(self, '_eye_cache', None) is None or self._eye_cache[0] != key:
            self._eye_cache = (key, torch.eye(G, dtype=torch.float32, device=device).repeat(nb, 1).contiguous())
        return self._eye_cache[1]

    def _plan(self, data: Dict, maskw, how, reduced: bool, piped: bool) -> "_Plan":
        """Every decision of one step, taken before its first launch: sizes, cached tables, the argument checks and the
        forms the stages below branch on.  ``how``: (normalize_first, train, opt_step) of ``run``; ``reduced``: a
        data-parallel step (with an all-reduce); ``piped``: one step of a pipelined chain."""
        tr = self.tr
        normalize_first, train, opt_step = how
        bank, nb = tr.net, tr.num_bands
        G, n = bank.num_groups, bank.num_delay_lines_per_group
        z, rows = data['z_values'], data['row_index']
        Btot = rows.numel()
        if Btot % nb:
            raise ValueError("the batch must hold the same number of receivers for every band")
        Bper, K, win = Btot // nb, z.shape[-1], tr.stft_win
        side2 = tr._stream('_side2') is not None
        gridK = FrequencyGrid.of(z)
        order = ops.irfft_slot_order(K, z.device) if (tr.use_slot_order and 'dataset' in data) else None
        # (receiver counts beyond what the sums over a band's receivers take fall through to the stored-signal chain)
        lin = (self.linear_transforms and not piped and ops.lin_supported(Bper, G)
               and hasattr(data.get('dataset'), 'direct_time'))
        start, length = tr._decay_window(K)
        # bands whose longest decay times differ have their own EDC windows (reference trainer.py:56-59): per-item window
        # lengths for the EDC scans, ``maskw`` then holds one pre-normalised row per band
        item_len, band_len = tr._item_windows(K, Bper, z.device)
        if item_len is not None and (maskw is None or maskw.ndim != 2):
            raise ValueError("bands with different EDC windows: pass the (bands, window) weight rows of "
                             "BandBankTrainer._band_mask_rows as maskw")
        pairs = order is not None and tr.use_pairs and win == 4096
        # blocks of 5..8 lines: the same step on the 17-polynomial records of csrc/blocktf8.hip (evaluation on the matrix
        # cores; unit-circle grids)
        big = n > 4
        if big and (gridK.logr is not None):
            raise NotImplementedError("blocks of more than four lines: the explicit step takes grids on the unit circle "
                                      "(set BandBankTrainer.use_fused = False to step this bank through the per-bin "
                                      "elimination kernels under autograd)")
        tail_ok = self.fused_tail and train and opt_step and not reduced and not piped and side2
        use_tail = tail_ok and not big
        # the normalisation scale joins the group signals behind the transform: energy pass on the side stream
        late = self.scale_late and lin and order is not None and normalize_first and not big and side2
        # blocks of 5..8 lines, integer delay lengths on the reference's own grid: normalize, the colorless pass and both
        # adjoints as real transforms of the coefficient sequences (csrc/polyfft.hip), normalize and the colorless pass on the
        # side stream; the forward group responses stay on the matrix-core pass (the dB stages of the decay losses need its
        # rounding: see that file).  The scale joins behind the transform, as ``late`` for the 4-line blocks
        tfp = None
        if big and self.transform_polys and lin and order is not None and gridK.rfft_nfft and side2 and normalize_first:
            T_seq = ops.tfp_plan(bank.delays, n, gridK.rfft_nfft)
            sob = ops.tfp_slot_of_bin(K, z.device)
            if T_seq is not None and sob is not None:
                tfp = (gridK.rfft_nfft, sob, T_seq)
        late8 = tfp is not None
        use_tail8 = tail_ok and late8                 # (8-line blocks: csrc/blocktf8.hip k_tf8_tail)
        spec = (lin and self.spectral_edr and pairs and ops.spec_supported(Bper, G)
                and hasattr(data['dataset'], 'direct_stft'))
        Hh, n_hidden = bank._mlp_cfg[0], bank._mlp_cfg[1]
        parts_in_mlp = ops.mlp_bwd_takes_parts(bank._freq_pi.numel(), Hh, n_hidden, G, Bper)
        if piped and (not train or reduced or not opt_step or not side2):
            raise ValueError("a pipelined step is a single-process training step with its optimiser update")
        if big:
            # (the previous step's tail left the rotations of the current blocks and the snapshot of the output gains)
            keep_records = use_tail8 and self.records_ok()
        else:
            # (the fused tail of the previous training step left them; anything else that touched M, b, c since made the
            # bookkeeping say so.  A training step WITHOUT the fused tail always evaluates them: captured into a graph it
            # would otherwise replay on records nobody refreshes)
            keep_records = self.records_ok() and (use_tail or not train)
        return _Plan(
            nb=nb, G=G, n=n, K=K, Ku=(K + 1) // 2 if K % 2 == 1 else K, Btot=Btot, Bper=Bper, win=win, start=start,
            length=length, order=order, tfp=tfp, item_len=item_len, band_len=band_len,
            sot=ops.irfft_slot_of_time(K, z.device) if (lin and train and order is not None) else None,
            train=train, normalize_first=normalize_first, opt_step=opt_step, reduced=reduced, piped=piped, big=big, lin=lin,
            pairs=pairs, spec=spec, late=late, late8=late8, use_tail=use_tail, use_tail8=use_tail8, keep_records=keep_records,
            parts_in_mlp=parts_in_mlp,
            # the normalisation scale inside the receiver gains (scale_late above)
            gfold=(late or late8) and not piped and spec and train and parts_in_mlp,
            # the output stage inside the transform's first pass (the stored-signal chain at the sizes that kernel takes)
            fold=pairs and K == 65537 and Bper % 2 == 0 and G <= 4 and not lin,
            # the colorless pass behind the EDC launches (see _colorless)
            late_colorless=big or spec,
            edc_one=self.edc_one_launch and ops.edc_lin_one_supported(length, G),
            # (a bank with the reference's per-band networks runs the gain network in front of the energy pass: _side_head)
            net_first=bool(getattr(bank, 'mixed_networks', False)))

    def _begin(self, p: "_Plan", data: Dict, maskw, inv: float, calls: Dict) -> "_Step":
        """The state the stages hand on: streams, events, the keep list, the step's inputs (``calls``: run's callables)"""
        tr = self.tr
        bank, z = tr.net, data['z_values']
        if p.lin:
            zu, direct = (data['dataset'].slot_grid(*p.order) if p.order is not None else z[:p.Ku]), None
        elif p.order is not None:
            zu, direct = data['dataset'].slot_ordered(*p.order)
        else:
            zu, direct = z[:p.Ku], data['target_early_response'][:, :p.Ku]
        return _Step(
            **calls, data=data, rows=data['row_index'], maskw=maskw, inv=inv, keep=self._keep,
            main=torch.cuda.current_stream(), side=tr._stream('_side'), side2=tr._stream('_side2'),
            M=bank._blocks().detach(), b=bank.input_gains.data.view(-1), c=bank.output_gains.data.view(-1),
            delays=bank.delays, ig=bank.inv_gamma, w=bank.output_scalars_w.detach(), gridK=FrequencyGrid.of(z), zu=zu,
            direct=direct, inv_world=shard_loss_scales(tr.world_size, 1, 1.0)['colorless'],
            T_edr=data['edr_target'][1], sum_abs=data['edr_target'][2], T_edc=data['edc_target'][1],
            ev={k: torch.cuda.Event() for k in ('start', 'g', 'h', 'mlp', 'mask', 'norm', 'x', 'edc', 'side', 'grg', 'mlpb')})

    def _gain_network(self, st: "_Step", out=None):
        """Receiver gains of the batch (gain_filters.py:497-536) -> (gains, xhat, rstd)"""
        bank = self.tr.net
        Hh, n_hidden, _, lo, hi = bank._mlp_cfg
        return ops.mlp_gains_fwd(st.data['norm_listener_position'], bank._freq_pi, st.w, Hh, n_hidden, bank.num_groups, lo, hi,
                                 st.rows, self.tr.num_bands, out=out)

    def _wait_gains(self, st: "_Step"):
        """main waits for the receiver gains of the side stream (a chained step: of the previous step's side stream)"""
        if st.pipe is None:
            st.main.wait_event(st.ev['mlp'])
        elif st.pipe.ready is not None:
            st.main.wait_event(st.pipe.ready)

    # ---- the stages, in the order ``run`` issues them ---------------------------------------------------------------------
    def _records_head(self, p: "_Plan", st: "_Step"):
        """main: records of the raw blocks [-> group responses of the late forms] [-> energy pass -> finish (normalize,
        trainer.py:317-332)]; records ev['start'] (the side stream's fork) and ev['norm'].
        The records are taken at the gains BEFORE the rescale and scaled afterwards: T is bilinear in b, c,
        T(b', c') = scale T(b, c).
        (the head is a serial chain on the main stream: forking the rotations off it and joining again costs more
        than the 10 us they take.  Captured BEFORE the fork of _side_head: the graph lays its hardware queues out along a
        depth-first walk of the nodes in capture order, and the chain captured first keeps its queue through every
        later join -- a chain that changes queue pays ~10 us per change)"""
        ev, keep, late_any = st.ev, st.keep, p.late or p.late8
        if not late_any:
            # (the side stream's head -- receiver gains, mask -- needs nothing of this step: forked off BEFORE the records launch,
            # so that the main chain's launches below stay first in capture order and keep its hardware queue)
            ev['start'].record()
        st.c_head = st.c
        if p.big:
            if p.keep_records:
                st.Q, st.QQ, st.c_head = self._records()
            else:
                st.Q, st.QQ = ops.ortho_fwd(st.M, True, True)
                if p.late8:
                    # the side stream's normalize rescales the gains in place while the main stream's pass reads them: a
                    # snapshot
                    st.c_head = st.c.detach().clone()
                    keep.append(st.c_head)
            st.coef, st.coef_sub = ops.tf8_coefs(st.QQ, st.ig, st.b, st.c, A1=st.M)
        else:
            if not p.keep_records:
                ops.tf_ortho_coefs(st.M, st.ig, st.b, st.c, out=self._records())
            st.Q, st.QQ, st.coef, st.coef_sub = self._records()
        self._rec_valid = False               # (until this step's end says otherwise)
        if late_any:
            ev['start'].record()              # (the side stream's energy pass reads the raw blocks' records)
        st.gridU = FrequencyGrid.of(st.zu)
        st.filt = self.tr._filter_on(p.Ku, p.order)
        gridK, gridU = st.gridK, st.gridU
        if p.late:
            # the main chain's first launch is captured BEFORE anything is forked off: the graph lays its hardware queues out
            # along the capture order, and a chain whose head is captured behind a side stream's first launch starts every
            # replay on the second queue (measured: 29 us between the last kernel of a step and the group responses of the
            # next one, against ~6)
            st.Hg, st.Ts = ops.tf_compose_fwd(gridU.turns, gridU.logr, st.coef, st.delays, p.n,
                                              self._eye_rows(p.nb, p.G, st.rows.device), None, None, st.filt, None, p.nb,
                                              save_T=True, want_H=True)
        if p.late8:
            # (as above: captured before the fork.  The grid in bin order -- T and 1 / Q where the adjoint's spectra are formed
            # --, the group responses through the band's filter scattered to the transform's slot order; unscaled: the
            # snapshot of the gains)
            st.Ts, _, st.Hg, st.Dinv8 = ops.tf8_tsave(gridK.turns[:p.Ku], st.coef, st.delays, p.n, st.c_head, None, p.nb, p.G,
                                                      quad=False, filt=st.filt, want_H=True, hslot=p.tfp[1])
            keep.append(st.Dinv8)
        if p.normalize_first and not late_any:
            # (captured in front of the side stream's first launch: see above)
            if p.big:
                _, st.scale = ops.tf8_energy(gridK.turns, st.coef_sub, st.delays, p.n, st.b, st.c, dturn=gridK.dturn)
            else:
                _, st.scale = ops.tf_energy(gridK.turns, gridK.logr, st.coef_sub, st.delays, p.n, st.b, st.c,
                                            want_energy=False, dturn=gridK.dturn)
        if not late_any:
            ev['norm'].record()

    def _side_head(self, p: "_Plan", st: "_Step"):
        """side2: [energy pass (normalize) of the late forms, gain network, finish] -> receiver gains -> mask draw; records
        ev['norm'] (late forms), ev['mlp'], ev['mask']"""
        ev, keep, gridK, pipe = st.ev, st.keep, st.gridK, st.pipe
        energy = (gridK.turns, gridK.logr, st.coef_sub, st.delays, p.n, st.b, st.c)
        with st.on_side2():
            if pipe is None or pipe.first:
                torch.cuda.current_stream().wait_event(ev['start'])
            if p.gfold and p.big:
                # 8-line blocks: the gain network FIRST (it needs nothing of this step), the transforms and the energy pass behind
                # it; the finish launch stores the gains times the scale -- rgain, what the step's launches take; rgain0, the
                # network's own output, is what its backward reads.  (4-line blocks: in front of the energy pass it measured
                # 0.355 against 0.352 ms, the same as no fold at all)
                st.rgain0, st.xhat, st.rstd = self._gain_network(st)
                keep.append(st.rgain0)
            if p.late:
                if p.gfold:
                    # (4-line blocks: the pass over the bins, the gain network, then the finish with the gains.  A bank with
                    # the reference's per-band networks -- three bands of 3 x 128 neurons -- runs the network FIRST: its
                    # launch is the longer of the two (33 us alone, 76 beside the energy pass and the transform passes when
                    # it started behind the pass: the EDR launch waited 45 us for the gains))
                    if p.net_first:
                        st.rgain0, st.xhat, st.rstd = self._gain_network(st)
                    st.ework = ops.tf_energy(*energy, phase=1, dturn=gridK.dturn)
                    if not p.net_first:
                        st.rgain0, st.xhat, st.rstd = self._gain_network(st)
                    keep.append(st.rgain0)
                    _, st.scale, st.rgain = ops.tf_energy(*energy, want_energy=False, work=st.ework, phase=2,
                                                          dturn=gridK.dturn, gains=st.rgain0, G=p.G)
                else:
                    _, st.scale = ops.tf_energy(*energy, want_energy=False, dturn=gridK.dturn)
                ev['norm'].record()
            elif p.late8:
                nblk8 = p.nb * p.G
                st.Xsub = ops.tfp_forward(st.coef_sub, st.delays, st.c, p.n, p.tfp[0], p.tfp[2])
                if p.gfold:
                    _, st.scale, st.rgain = ops.tfp_energy(st.Xsub[:nblk8], st.Xsub[nblk8:], p.n, st.b, st.c, gains=st.rgain0,
                                                           G=p.G)
                else:
                    _, st.scale = ops.tfp_energy(st.Xsub[:nblk8], st.Xsub[nblk8:], p.n, st.b, st.c)
                ev['norm'].record()
                keep.append(st.Xsub)
            if p.gfold:
                ev['mlp'].record()
            elif pipe is None:
                st.rgain, st.xhat, st.rstd = self._gain_network(st)
                ev['mlp'].record()
            else:
                # the previous step of the chain (or the prologue) has left this step's receiver gains in the pipe
                st.rgain, st.xhat, st.rstd = pipe.cur
            # the EDC time mask is drawn on the stream that runs the EDC scans.  (Drawn on `side`, with the reported
            # total on `side` waiting for the sums of `side2`, the two forked streams depend on each other in both
            # directions -- hipStreamEndCapture of ROCm 7.2 segfaults on that topology.)
            if st.mask_draw is not None:
                st.mask_draw()
            ev['mask'].record()

    def _group_signals(self, p: "_Plan", st: "_Step"):
        """main (time-domain output stage): group responses through the band's filter -> G time signals per band; the
        receivers' signals are formed from them and the dataset's transformed direct paths in one streaming pass
        (csrc/linear.hip)"""
        gridU, K = st.gridU, p.K
        st.eye = self._eye_rows(p.nb, p.G, st.rows.device)
        st.xd = st.data['dataset'].direct_time(self.tr.subband_filter_freq_resp, K)
        if p.late8:
            pass                          # (launched by _records_head)
        elif p.big:
            # (the group responses through the band's filter written by the same launch: no tensor operation between the
            # transfer functions and the transform)
            st.Ts, _, st.Hg, st.Dinv8 = ops.tf8_tsave(gridU.turns, st.coef, st.delays, p.n, st.c, st.scale, p.nb, p.G,
                                                      quad=False, filt=st.filt, want_H=True)
            st.keep.append(st.Dinv8)
            st.ev_ts = torch.cuda.Event()
            st.ev_ts.record()
        elif not p.late:
            st.Hg, st.Ts = ops.tf_compose_fwd(gridU.turns, gridU.logr, st.coef, st.delays, p.n, st.eye, st.scale, None,
                                              st.filt, None, p.nb, save_T=True, want_H=True)
        if p.gfold:
            st.tau = ops.irfft_odd_fwd(st.Hg, K, slots=True, pairs=True)     # (signals of the unscaled functions: no wait)
        elif p.late or p.late8:
            # (the wait sits in front of the LAST pass, the only reader of the scale)
            st.tau = ops.irfft_odd_fwd(st.Hg, K, slots=True, pairs=True, oscale=st.scale,
                                       before_last=lambda: st.main.wait_event(st.ev['norm']))
        else:
            st.tau = ops.irfft_odd_fwd(st.Hg, K, slots=p.order is not None, pairs=p.order is not None)
        st.H = st.Hg
        st.keep.extend((st.tau, st.xd))

    def _stored_output_stage(self, p: "_Plan", st: "_Step"):
        """main (stored-signal chain): H = (sum_g rgain s_g T_g + direct) filt per receiver -- or, folded, only the saved
        group transfer functions: _receiver_signals then forms H inside the transform's first pass"""
        gridU = st.gridU
        # the receiver gains come from the side stream: with the output stage folded into the transform the transfer-function
        # launch below does not read them, and the wait goes behind it -- by then the event was signalled long ago (a wait on
        # a signalled event is free; in front of the launch the idle main stream paid a cross-queue wake-up of ~12 us)
        if not p.fold:
            self._wait_gains(st)
        if p.big:
            st.Ts, Tq8 = ops.tf8_tsave(gridU.turns, st.coef, st.delays, p.n, st.c, st.scale, p.nb, p.G, quad=True)
            # (the colorless pass of the 8-line blocks is VALU-bound like this launch: it starts behind it and runs
            # beside the memory-bound transform instead -- measured: tsave 105 -> 55 us in the step)
            st.ev_ts = torch.cuda.Event()
            st.ev_ts.record()
            if p.fold:
                st.H = Tq8
            else:
                # (sizes the folded transform does not take: the output stage as tensor operations -- small grids only)
                Hs = torch.einsum('qbg,qgk->qbk', st.rgain.reshape(p.nb, p.Bper, p.G).to(torch.complex64),
                                  st.Ts.reshape(p.nb, p.G, -1))
                Hs = Hs + st.direct[st.rows].reshape(p.nb, p.Bper, -1)[..., :st.Ts.shape[1]]
                if st.filt is not None:
                    Hs = Hs * st.filt.reshape(p.nb, 1, -1)
                st.H = Hs.reshape(p.Btot, -1).contiguous()
        else:
            st.H, st.Ts = ops.tf_compose_fwd(gridU.turns, gridU.logr, st.coef, st.delays, p.n, st.rgain, st.scale, st.direct,
                                             st.filt, st.rows, p.nb, save_T=True, want_H=not p.fold)
        if p.fold:
            st.Tq, st.H = st.H, None

    def _colorless(self, p: "_Plan", st: "_Step"):
        """side2: colorless pass (spectral loss + dL/drecords of the sub-FDNs, sparsity) -> st.grec_sub, st.out3, st.gQ;
        records ev['side'].  Blocks of <= 4 lines on the stored-signal chain: in front of the scans, beside the output
        stage and the transform (behind the scans it ran beside the STFT adjoint: same step time either way, measured).
        Blocks of 5..8 lines: BEHIND the scans -- the pass takes ~200 us there, and in front of them the EDC gradient
        reached the odd-frame launch of the STFT adjoint late.  Composed-spectra step: the same holds for the small
        blocks -- in front of the scans the VALU-bound pass ran beside the latency-bound transforms of the G group
        signals, which sit on the critical chain: 18.6 against 9.6 us for the row pass; behind them it runs beside the
        memory-bound EDR kernels"""
        cfg, gridK, weight = self.tr.config, st.gridK, self.tr.config.spectral_loss_weight * st.inv_world
        with st.on_side2():
            if not p.late and not p.late8:         # (recorded on this very stream: no wait -- a captured wait of a stream
                torch.cuda.current_stream().wait_event(st.ev['norm'])      # for its own event is asking for trouble)
            if p.late8:
                nblk8 = p.nb * p.G
                grec_sub, loss_g = ops.tfp_colorless(st.Xsub[:nblk8], st.Xsub[nblk8:], p.tfp[0], p.n, st.delays, st.scale,
                                                     cfg.use_asym_spectral_loss, weight, T=p.tfp[2])
            elif p.big:
                torch.cuda.current_stream().wait_event(st.ev_ts)
                grec_sub, loss_g = ops.tf8_colorless(gridK.turns, st.coef_sub, st.delays, p.n, st.c, st.scale,
                                                     cfg.use_asym_spectral_loss, weight, dturn=gridK.dturn)
            else:
                grec_sub, loss_g = ops.tf_colorless(gridK.turns, gridK.logr, st.coef_sub, st.delays, p.n, st.scale,
                                                    cfg.use_asym_spectral_loss, weight, dturn=gridK.dturn)
            st.out3, st.gQ = ops.colorless_terms(loss_g, st.Q, cfg.spectral_loss_weight, cfg.sparsity_loss_weight,
                                                 st.inv_world, want_grad=p.train, nbands=p.nb)
            st.ev['side'].record()
        st.grec_sub = grec_sub
        st.keep.extend((grec_sub, loss_g, st.out3, st.gQ))

    def _receiver_signals(self, p: "_Plan", st: "_Step") -> torch.Tensor:
        """main: the receivers' time signals of the stored-signal decay losses"""
        if p.lin:
            self._wait_gains(st)
            return ops.lin_combine_fwd(st.xd, st.rows, st.tau, st.rgain, p.nb, p.K, p.order is not None, p.pairs)
        if p.fold:                        # (the output stage rides the transform's first pass: H is never stored)
            self._wait_gains(st)
            x2, h0 = ops.irfft_odd_pairs_compose_fwd(st.direct, st.rows, st.Tq, st.rgain, st.filt, p.K, p.nb)
            st.keep.extend((h0, st.Tq))
            return x2
        if p.pairs:
            return ops.irfft_odd_fwd(st.H, p.K, slots=True, pairs=True)
        return ops.irfft_odd_fwd(st.H, p.K, slots=p.order is not None)

    def _decay_stored(self, p: "_Plan", st: "_Step"):
        """One chain over the whole batch: main: irfft -> STFT -> EDR -> STFT adjoint (even frames, then odd frames +
        EDC gradient) -> irfft adjoint; side2: EDC scans.  Records ev['x'] / ev['edc'] / ev['g']; leaves st.li_edr,
        st.li_edc and st.gH = dL/dH -- on the time-domain output stage the chain stops at dL/dx: (g, None)
        (pair-interleaved, merged) or (g_edc, g_edr)."""
        cfg, keep, ev, main = self.tr.config, st.keep, st.ev, st.main
        K, Btot, win, train = p.K, p.Btot, p.win, p.train
        x = self._receiver_signals(p, st)
        ev['x'].record()
        if p.pairs:
            P = ops.stft_power_pairs(x, Btot, win)
            g_edr = None
        else:
            g_edr = torch.empty_like(x) if train else None
            P = ops.stft_power(x, win, zero_buf=g_edr)
        with st.on_side2():
            torch.cuda.current_stream().wait_event(ev['x'])
            if p.pairs:
                li_edc, g_edc = ops.edc_loss_pairs(x, Btot, p.start, p.length, st.T_edc, st.maskw, st.inv, cfg.edc_loss_weight,
                                                   train, rows=st.rows, item_len=p.item_len, items_per_band=p.Bper)
            else:
                li_edc, g_edc = ops.edc_loss(x, p.start, p.length, st.T_edc, st.maskw, st.inv, cfg.edc_loss_weight, train,
                                             rows=st.rows, item_len=p.item_len, items_per_band=p.Bper)
            ev['edc'].record()
        li_edr = ops.edr_loss(P, st.T_edr, st.sum_abs, None, cfg.edr_loss_weight, train, rows=st.rows, defer=True)
        keep.extend((x, P, g_edr, li_edc, g_edc, li_edr))
        gH = None
        if train:
            if p.pairs:
                # even frames first, alone; the EDC gradient joins with the odd frames (the EDC scans are the
                # longer of the two branches: the main stream would otherwise sit idle until they finish)
                g = ops.stft_power_pairs_bwd(x, Btot, win, P, phase=0)
                main.wait_event(ev['edc'])
                ops.stft_power_pairs_bwd(x, Btot, win, P, base=g_edc, out=g, phase=1)
                ev['g'].record()
                gH = (g, None) if p.lin else ops.irfft_odd_pairs_bwd(g, K, Btot)
                keep.append(g)
            else:
                g_edr = ops.stft_power_bwd(x, win, P, g_edr)
                main.wait_event(ev['edc'])
                ev['g'].record()
                if p.lin:
                    gH = (g_edc, g_edr)
                else:
                    gH = ops.irfft_odd_bwd(g_edc, K, (K + 1) // 2 if p.order is not None else st.H.shape[1], g_edr,
                                           slots=p.order is not None)
            keep.append(gH)
        else:
            main.wait_event(ev['edc'])
            ev['g'].record()
        st.li_edr, st.li_edc, st.gH = li_edr, li_edc, gH

    def _decay_spec(self, p: "_Plan", st: "_Step"):
        """The decay losses without per-receiver transforms of any kind (csrc/edrlin.hip, xlin_dev.h):
            main : STFT of the band's G group signals -> EDR loss on composed spectra (loss partials, EDR part of
                   dL/drgain) -> gradient spectra summed over the band's receivers -> their adjoint STFT (EDR part of dL/dtau)
            side2: EDC term on samples formed where they are read (-> dL/dx of the EDC term) -> its sum over the band's
                   receivers (EDC part of dL/dtau)
        Records ev['x'] / ev['edc'] (/ ev['g']: validation only); leaves st.li_edr partials, st.li_edc and, training,
        st.g_edc, st.gam_edr, st.parts."""
        tr, cfg, keep, ev = self.tr, self.tr.config, st.keep, st.ev
        nb, G, K, win, train = p.nb, p.G, p.K, p.win, p.train
        rows, rgain, tau, ds, tiled = st.rows, st.rgain, st.tau, st.data['dataset'], self.tiled_spectra
        Sd = ds.direct_stft(tr.subband_filter_freq_resp, K, win, tiled=tiled)
        T_edr = ds.edr_target_tiled() if tiled else st.T_edr
        ev['x'].record()                                     # (tau complete)
        nch = 1 if p.edc_one else ops.lin_gamma_dots_tiles(K)
        parts = None
        if train:
            # partial rows of dL/drgain: [EDC dot products | EDR columns]; the gain network's backward sums them
            parts = torch.empty((p.Btot * G, nch + ops.edr_lin_parts(win // 2 + 1, fused=self.edr_one_launch)),
                                dtype=torch.float32, device=rows.device)
        Stau = ops.stft_pairs_spectrum(tau, nb * G, win, tiled=tiled)
        with st.on_side2():
            torch.cuda.current_stream().wait_event(ev['x'])
            edc_args = (st.xd, rows, tau, rgain, nb, K, p.start, p.length, st.T_edc, st.maskw, st.inv, cfg.edc_loss_weight,
                        train)
            if p.edc_one:
                # ONE launch, one workgroup per receiver: loss, dL/dx on the window (plain rows) and the EDC column of
                # ``parts``
                li_edc, g_edc = ops.edc_lin_one(*edc_args, trows=rows, item_len=p.item_len, dots=parts, col=0)
                if train:
                    # the EDC part of dL/dtau right here, beside the EDR launch: the main chain then merges three small
                    # signal sets behind the adjoint STFT instead of sweeping the receivers' gradient rows (42 MB) there
                    g_edc = (g_edc, ops.lin_gamma_win(g_edc, rgain, nb, K, p.start, p.length, band_win_len=p.band_len))
            else:
                li_edc, g_edc = ops.edc_loss_pairs_lin(*edc_args, trows=rows, item_len=p.item_len, fill_outside=False)
            ev['edc'].record()
        self._wait_gains(st)
        gP = Gs = None
        if train and self.edr_one_launch:
            li_edr, Gs = ops.edr_lin_loss_gsum(Sd, rows, Stau, rgain, nb, T_edr, st.sum_abs, cfg.edr_loss_weight, dots=parts,
                                               col0=nch, tiled=tiled, nsplit=self._edr_runs(nb, p.Bper))
        else:
            li_edr, gP = ops.edr_lin_loss(Sd, rows, Stau, rgain, nb, T_edr, st.sum_abs, cfg.edr_loss_weight, train,
                                          dots=parts, col0=nch, tiled=tiled)
        if not train:
            # (training: the side stream's consumers of the EDR partials wait for the LATER event behind the gamma merge --
            # one edge from the main chain to the side stream instead of two; an edge costs the main chain ~4 us)
            ev['g'].record()                                 # (EDR partials complete)
        keep.extend((Sd, Stau, li_edc, g_edc, li_edr, gP, parts))
        st.li_edr, st.li_edc, st.gH = li_edr, li_edc, None
        if not train:
            st.main.wait_event(ev['edc'])
            return
        if Gs is None:
            Gs = ops.edr_lin_gsum(Sd, rows, Stau, rgain, nb, gP)
        # (one launch for all frames: the odd frames' contributions go to a second signal set that the gamma merge adds)
        gam_edr = ops.stft_pairs_spectrum_bwd(Gs, K, nb * G, win, tiled=tiled, split_parity=True)
        keep.extend((Gs, gam_edr))
        st.g_edc, st.gam_edr, st.parts = g_edc, gam_edr, parts

    def _report(self, p: "_Plan", st: "_Step"):
        """the reported sums and total (off the gradient path)"""
        cfg = self.tr.config
        s_ = ops.weighted_sums(st.li_edr, cfg.edr_loss_weight, st.li_edc, cfg.edc_loss_weight, st.sum_abs, st.rows, p.nb)
        st.sums, st.total = s_, ((s_[:, 0] + st.out3[:, 0]) if p.nb > 1 else (s_[0] + st.out3[0]))

    def _adjoint_signals(self, p: "_Plan", st: "_Step"):
        """main (time-domain output stage): gamma_g = sum_b rgain[b][g] dL/dx[b] (G signals per band) -> their adjoint
        transform = dL/d(T_g filt) -> st.gH_rec, st.rg_rec: the records pass at "B = G receivers with identity gains".
        Composed spectra: records st.ev_gam behind the gamma launch."""
        K, nb, keep = p.K, p.nb, st.keep
        if not p.lin:
            st.gH_rec, st.rg_rec = st.gH, st.rgain
            return
        tau_pairs = p.order is not None
        if p.spec:
            # dL/dtau = [EDC part: sum_b rgain dL/dx_b of the scans] + [EDR part: adjoint STFT of the band's G
            # gradient spectra, already summed over the receivers]
            st.gsig, st.gsig_b = st.g_edc, None
            st.main.wait_event(st.ev['edc'])
            ge_a, ge_b = st.gam_edr if isinstance(st.gam_edr, tuple) else (st.gam_edr, None)
            if isinstance(st.gsig, tuple):         # (rows, their sums per group: the one-launch EDC term)
                gam = ops.lin_merge_slots(st.gsig[1], ge_a, ge_b, p.sot)
            else:
                # one sweep over the EDC gradient signals (their window only): the G sums per band AND the EDC part
                # of dL/drgain
                gam = ops.lin_gamma_dots(st.gsig, st.rgain, nb, K, st.tau, st.parts, p.start, p.length, base=ge_a,
                                         slot_of_time=p.sot, band_win_len=p.band_len, base_b=ge_b)
            st.ev_gam = torch.cuda.Event()
            st.ev_gam.record()
        else:
            st.gsig, st.gsig_b = st.gH
            gam = ops.lin_gamma(st.gsig, st.rgain, nb, K, p.pairs, tau_pairs, gxb=st.gsig_b, slot_of_time=p.sot)
        if tau_pairs:
            gHg = ops.irfft_odd_pairs_bwd(gam, K, nb * p.G, tslots=p.sot is not None)
        else:
            gHg = ops.irfft_odd_bwd(gam, K, p.Ku, None, slots=False)
        keep.extend((gam, gHg, st.eye))
        st.gH_rec, st.rg_rec = gHg, st.eye

    def _records_pass(self, p: "_Plan", st: "_Step"):
        """main: dL/dH (or the adjoint spectra of the group signals) -> partial rows of dL/drecords (st.grec)"""
        gridU = st.gridU
        if p.late8:
            st.grec = ops.tfp_compose_bwd(p.tfp[0], p.nb, p.G, p.n, st.delays, p.Ku, p.tfp[1], st.gH_rec, st.filt, st.Ts,
                                          st.Dinv8, tscale=st.scale, gain_fold=p.gfold, T=p.tfp[2])
        elif p.big:
            # (the linear step's adjoint runs on the grid of the forward pass: its saved T' and 1 / Q come back)
            st.grec = ops.tf8_compose_bwd(gridU.turns, st.coef, st.delays, p.n, st.c, st.scale, st.rg_rec, st.gH_rec, st.filt,
                                          p.nb, saved=(st.Ts, st.Dinv8) if p.lin else None)
        else:
            st.grec = ops.tf_compose_bwd(gridU.turns, gridU.logr, st.coef, st.delays, p.n, st.rg_rec, st.gH_rec, st.Ts, st.filt,
                                         p.nb, partial=True, tscale=st.scale if p.late else None,
                                         gain_fold=p.gfold and p.late)

    def _side_backward(self, p: "_Plan", st: "_Step"):
        """side2: reported sums -> gains pass (dL/drgain) -> gain network backward [-> its Adam range] -> ``tail`` (the next
        step's receivers) [-> a chained step: the next step's receiver gains]; records ev['mlpb'].
        The reported sums go in front of the gains pass (their inputs are long complete; behind it they would sit on
        the path to Adam)."""
        tr, ev, pipe = self.tr, st.ev, st.pipe
        bank, opt, nb, G = tr.net, tr.optimizer, p.nb, p.G
        Hh, n_hidden, _, lo, hi = bank._mlp_cfg
        with st.on_side2():
            cur = torch.cuda.current_stream()
            cur.wait_event(st.ev_gam if p.spec else ev['g'])         # (composed spectra: behind the EDR launch as well)
            self._report(p, st)
            if st.allreduce is not None:
                # data-parallel: this rank's loss terms ride the gradient bucket -- [EDR | EDC | colorless share]
                # per band behind the gradients -- and ONE all-reduce sums both over the ranks.
                # Written here, off the path: the main stream's wait for this branch covers it
                slots = opt.extra.view(3, nb)
                torch.stack((st.sums.reshape(nb, 3)[:, 1], st.sums.reshape(nb, 3)[:, 2], st.out3.reshape(nb, 3)[:, 0]),
                            out=slots)
            grg = None
            if p.lin:
                # dL/drgain[b][g] = <dL/dx[b], tau_g>: partial rows over the time samples
                if p.spec:        # (the EDR part of the rows was left by the EDR kernel, the EDC part by the EDC launch)
                    # behind the gamma pass: both stream the same 59 MB, and the gamma pass heads the critical chain
                    # (side by side: 40 us for it instead of 15)
                    cur.wait_event(st.ev_gam)
                    ggp = st.parts
                else:
                    ggp = ops.lin_gain_dots(st.gsig, st.tau, nb, p.Btot, G, p.K, p.pairs, p.order is not None, gxb=st.gsig_b)
                if not p.parts_in_mlp:
                    grg, ggp = ops.tf_rows_sum(ggp).view(p.Btot, G), None
            else:
                cur.wait_event(ev['grg'])
                if p.parts_in_mlp:
                    # the gains pass leaves its per-chunk partial rows; every receiver's wave of the gain network's
                    # backward sums its own (same order as the row-sum launch that sat between the two, on the path to
                    # the update)
                    ggp = ops.tf_gain_grad(st.Ts, st.gH, G, st.filt, nb, partial=True)
                else:
                    grg, ggp = ops.tf_gain_grad(st.Ts, st.gH, G, st.filt, nb), None
            ops.mlp_gains_bwd(st.data['norm_listener_position'], bank._freq_pi, st.w, Hh, n_hidden, G, lo, hi,
                              st.rgain0 if p.gfold else st.rgain, st.xhat, st.rstd, grg, st.rows, nb, out=self.g_w,
                              ggains_parts=ggp, colscale=st.scale if p.gfold else None)
            st.keep.append(ggp)
            if pipe is not None:
                # the gain network's range of the flat buffers is stepped HERE, behind its gradient, on this
                # stream; then the next step's receivers and its receiver gains -- the main stream never waits
                # for this branch again until the next output stage needs them
                opt.step_range(*self.w_range, second=True)
                if st.tail is not None:
                    st.tail()
                self._gain_network(st, out=pipe.nxt)
                pipe.ready_next = torch.cuda.Event()
                pipe.ready_next.record()
            else:
                if p.use_tail or p.use_tail8:
                    # the gain network's range of the flat buffers, straight behind its gradient on this stream (its
                    # own step counter: no ordering with the main stream's fused tail)
                    opt.step_range(*self.w_range, second=True)
                ev['mlpb'].record()
                if st.tail is not None:
                    st.tail()             # (every reader of ``rows`` is ordered before this point: main's are in
                                          # front of ev['grg'], this stream's are its own earlier launches)
        st.grg = grg

    def _parameter_tail(self, p: "_Plan", st: "_Step"):
        """main: records (partial rows of the records pass + the colorless pass's) -> dL/dM, dL/db, dL/dc: one launch
        [-> Adam on the blocks' own M, b, c -> the NEXT step's Q, Q Q and record sets / gain snapshot, in the same launch];
        then the optimiser update of a step without the fused tail"""
        tr, opt = self.tr, self.tr.optimizer
        rec = (st.QQ, st.ig, st.grec, st.grec_sub, st.b, st.c, st.M, st.gQ, st.Q, self.g_b, self.g_c)
        if p.use_tail8:
            ops.tf8_tail(*rec, self.g_M, opt, *self._off, *self._records())
        elif p.big:
            ops.tf8_param_grads(st.QQ, st.ig, st.grec, st.b, st.c, st.M, A1=st.M, part1=st.grec_sub, gQ=st.gQ, Q=st.Q,
                                gb=self.g_b, gc=self.g_c, gM=self.g_M)
        elif p.use_tail:
            ops.tf_tail(*rec, self.g_M.view(-1), opt, *self._off, *self._records())
        else:
            ops.tf_param_grads(st.QQ, st.ig, st.grec, st.b, st.c, st.M, A1=st.M, grec1=st.grec_sub, gQ=st.gQ, Q=st.Q,
                               gb=self.g_b, gc=self.g_c, gM=self.g_M)
        st.keep.extend((st.grg, st.grec))
        if p.piped:
            # everything but the gain network, straight behind its gradients
            opt.step_range(0, self.w_range[0], second=False)
            torch.autograd.graph.increment_version(opt._params)
            return
        opt._packed = True                            # the flat gradient buffer is complete
        if p.use_tail or p.use_tail8:
            # both ranges of the flat buffers are stepped (main: fused tail; side2: the gain network's own launch)
            opt._packed = False
            torch.autograd.graph.increment_version(opt._params)
            self._rec_valid, self._rec_versions = True, self._versions()
        elif p.opt_step and not p.reduced and st.side2 is not None:
            # single process: the update runs on the branch that finishes LAST (the gain network's backward), behind
            # an event of the main stream that was signalled earlier -- a wait on a long-signalled event is free,
            # while the main stream, idle when the side branch signals, would pay the 8-12 us of a cross-queue wake-up
            ev_pg = torch.cuda.Event()
            ev_pg.record()
            with st.on_side2():
                torch.cuda.current_stream().wait_event(ev_pg)
                self.finish(None)
        else:
            st.main.wait_event(st.ev['mlpb'])
            if p.opt_step:
                red = self.finish(st.allreduce)
                if red is not None:
                    st.sums, st.total = red

    def _losses(self, p: "_Plan", st: "_Step") -> Dict:
        col = (lambda t, i: t[:, i]) if p.nb > 1 else (lambda t, i: t[i])
        return {'edc_loss': col(st.sums, 2), 'edr_loss': col(st.sums, 1), 'spectral_loss': col(st.out3, 1),
                'sparsity_loss': col(st.out3, 2), '_total': st.total}

    def _end(self, p: "_Plan", st: "_Step") -> Dict:
        """Join of the side streams -> loss dict.  One step of a pipelined chain: no join with the side stream (only the
        chain's last step joins, which stream capture needs); this step's tensors stay referenced until the END of the next
        step -- by then every stream has passed a point ordered behind their last readers (the allocator hands a freed block
        only to the stream it was allocated on, but main-stream blocks are read on the side stream too)."""
        keep, pipe = st.keep, st.pipe
        keep.extend((st.sums, st.total))
        losses = self._losses(p, st)
        if pipe is None or pipe.last:
            for s_ in (st.side, st.side2):
                if s_ is not None:
                    st.main.wait_stream(s_)
        if pipe is not None:
            self._keep_prev = [] if pipe.last else list(keep)
            keep.clear()
            pipe.advance()
            return losses
        keep.clear()          # every consumer is ordered before the next step's first launch on each stream
        if not p.big and not p.train and not p.normalize_first:
            self._rec_valid, self._rec_versions = True, self._versions()      # (nothing touched M, b, c)
        return losses

    @torch.no_grad()
    def run(self, data: Dict, maskw: Optional[torch.Tensor], inv: float, normalize_first: bool, train: bool,
            allreduce=None, opt_step: bool = True, mask_draw=None, tail=None, pipe=None) -> Dict:
        """One step of every band on the band-major batch ``data`` (collate(lean="rows")).  ``maskw``: EDC time
        weights (None: no mask), ``inv``: what the EDC terms are divided by beyond the weights (1 when the weights are
        pre-normalised).  ``train``: gradients into the flat buffer, [all-reduce,] Adam (``opt_step=False`` stops in front
        of the all-reduce: the caller runs it and the update).  ``mask_draw``: callable that fills ``maskw`` on the
        device (run on the EDC stream, off the path to the output stage).  ``tail``: callable run on the side stream
        behind the last reader of the batch's receiver indices (GraphedTrainStep fetches the next step's there).
        ``pipe``: a :class:`StepPipe` -- this call is one step of a chain captured into one graph in which the side
        stream runs ahead (see the class).  Returns the loss dict of
        ``BandBankTrainer._step_losses`` (+ '_total').

        Scheduling rules (measured on the replayed graph, profiles/): a dependency that crosses streams costs
        8-12 us when the waiting stream is idle at the moment of the signal and nothing when the signal came earlier;
        and at a fork the graph keeps the FIRST captured successor on the producer's hardware queue.  So the critical
        chain stays on the main stream, its next kernel is captured before anything is forked off a node, and the
        side branches are arranged to finish early.  The host order of the stages below IS that schedule
        (tests/test_gpu_bankstep_order.py pins it)."""
        p = self._plan(data, maskw, (normalize_first, train, opt_step), allreduce is not None, pipe is not None)
        st = self._begin(p, data, maskw, inv, dict(allreduce=allreduce, mask_draw=mask_draw, tail=tail, pipe=pipe))
        self._records_head(p, st)         # main (captured BEFORE the fork: its first launch keeps the hardware queue)
        self._side_head(p, st)            # side2
        if p.lin:
            self._group_signals(p, st)
        else:
            self._stored_output_stage(p, st)
        st.keep.extend((st.coef_sub, st.ework, st.Q, st.QQ, st.coef, st.rgain, st.xhat, st.rstd, st.scale, st.H, st.Ts))
        if not p.late_colorless:
            self._colorless(p, st)        # side2
        # ---- decay losses: irfft -> STFT -> EDR -> STFT adjoint -> irfft adjoint, EDC scans beside them
        st.ev['h'].record()
        if p.spec:
            self._decay_spec(p, st)
        else:
            self._decay_stored(p, st)
        if p.late_colorless:
            self._colorless(p, st)        # side2, behind the EDC launches
        if not train:
            with st.on_side2():
                torch.cuda.current_stream().wait_event(st.ev['g'])
                self._report(p, st)
            return self._end(p, st)
        if (p.use_tail or p.use_tail8) and not torch.cuda.is_current_stream_capturing():
            self.tr.optimizer.sync_lr()       # (both Adam launches of the split update read the device table)
        # ---- backward of the output stage.  Its two passes are independent and both stream dL/dH: the records pass
        # stays on the main stream, the gains pass (-> gain network backward) runs beside it on side2 -- together
        # 50 us instead of 29 + 45 one after the other.
        st.ev['grg'].record()                 # (dL/dH complete)
        self._adjoint_signals(p, st)          # main
        self._records_pass(p, st)             # main
        self._side_backward(p, st)            # side2
        st.main.wait_event(st.ev['side'])     # (signalled long ago; dropping it measured no gain: 0.667 vs 0.663 ms)
        self._parameter_tail(p, st)           # main
        return self._end(p, st)

    # -- the part of a data-parallel step behind the gradients ------------------------------------------------------
    def finish(self, allreduce):
        """[all-reduce of the bucket,] Adam.  Returns (sums, total) rebuilt from the reduced loss slots -- the whole
        job's EDR / EDC terms and total per band -- or None for a single process."""
        tr = self.tr
        nb = tr.num_bands
        red = None
        if allreduce is not None:
            allreduce()
        tr.optimizer.step()                  # (straight behind the collective: the reported sums below are not on the path)
        if allreduce is not None:
            slots = tr.optimizer.extra.view(3, nb)
            total = slots.sum(dim=0)
            sums = torch.stack((total, slots[0], slots[1]), dim=1)          # [total, w_edr edr, w_edc edc] per band
            red = (sums, total) if nb > 1 else (sums[0], total[0])
        return red


class StepPipe:
    """State of a chain of explicit steps captured into ONE graph with the side stream running ahead of the main one.

    In a single step the main stream waits for the side stream twice where nothing but latency is gained or lost: at
    the head (the receiver gains of the batch, ~12 us behind the side stream's fork) and at the tail (Adam behind the
    gain network's backward, ~15 us), and every step ends with a join and starts with a fork (~11 us).  In a chain the
    side stream steps the gain network's parameters itself, fetches the next step's receivers and evaluates their gains
    right behind the gain network's backward of the current step; the main stream steps everything else straight
    behind its own last gradient kernel and goes on with the next step.  The numbers are those of the single steps,
    bit for bit (tests/test_gpu_bank.py).

    ``bufs``: two sets of (gains (B, G), xhat (B, nl, H), rstd (B, nl)) owned by the caller: step i of the chain reads
    set i % 2 and fills set (i + 1) % 2, so a chain of EVEN length leaves the next chain's first set filled."""

    def __init__(self, bufs, steps: int):
        if steps % 2:
            raise ValueError("a pipelined chain has an even number of steps")
        self.bufs, self.steps, self.i = bufs, steps, 0
        self.ready = None            # event behind the gains of the CURRENT step (None: produced before this chain)
        self.ready_next = None

    @property
    def cur(self):
        return self.bufs[self.i % 2]

    @property
    def nxt(self):
        return self.bufs[(self.i + 1) % 2]

    @property
    def first(self):
        return self.i == 0

    @property
    def last(self):
        return self.i == self.steps - 1

    def advance(self):
        self.i += 1
        self.ready, self.ready_next = self.ready_next, None
