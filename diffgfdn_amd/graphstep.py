"""Training steps captured into HIP graphs and replayed: ``GraphedTrainStep`` (a grid-of-receivers trainer's or a band
bank's step, read from dataset-level stores through a static index buffer), ``GraphedModuleStep`` (``train_step(batch)`` through
the model's own module) and ``DirectionalBank`` (several of the latter on lanes inside ONE graph).  All three capture the same
way -- ``_warm_up``, then the capture on the stream it ran on; the trainers import this module, never the other way round."""
import contextlib
from typing import Callable, Dict, Optional

import torch
import torch.distributed as dist

from . import hip_ops as ops
from .bankstep import StepPipe
from .functional import FrequencyGrid
from .losses import directional_edc_loss


def _warm_up(trainer, stream, step: Callable, also_reset: Optional[Callable] = None):
    """Three eager ``step()`` calls on ``stream`` that leave no trace: parameters and optimiser state are restored IN PLACE (the
    graph will reference these very tensors), ``also_reset`` puts back what else the steps advanced and the gradients are
    dropped.  The caller captures on ``stream``.  The stream rules, each learned the hard way (ROCm 7.2):
      * warm-up AND capture on ONE private stream: autograd pins every parameter's AccumulateGrad node to the stream of its
        first backward, and a capture that has to hop to another stream and back dies in hipStreamEndCapture -- a bank
        warms every band up on the lane it is captured on;
      * a capture over several lanes starts on the FIRST lane: a separate origin stream that only forks and joins makes
        hipStreamEndCapture segfault, and so does a forked lane that forks again (a trainer on a lane beside the first
        keeps its side branch on the lane itself)."""
    params = list(trainer.net.parameters())
    saved_p = [p.detach().clone() for p in params]
    saved_s = [t.detach().clone() for t in trainer.optimizer.state_tensors()]
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(3):
            step()
        for p, sp in zip(params, saved_p):
            p.data.copy_(sp)
        for t, st in zip(trainer.optimizer.state_tensors(), saved_s):
            t.copy_(st)
        if also_reset is not None:
            also_reset()
        trainer.optimizer.zero_grad(set_to_none=True)


def _pinned_grids():
    """The recorded launches hold raw pointers into the frequency grids (turns / log radius): a step keeps the grid objects
    alive as long as its graphs (the cache may drop them)."""
    return FrequencyGrid.live()


def _drain_for(*graphs):
    """``__del__`` of a step: a graph executable must not be destroyed while its last launch is still in flight (its
    kernel-argument buffers go with it) -- drain the device first."""
    try:
        if any(g is not None for g in graphs):
            torch.cuda.synchronize()
    except Exception:        # noqa: BLE001 -- interpreter shutdown
        pass


def _refresh(static: Dict, batch: Optional[Dict]):
    """The static batch a graph reads <- ``batch``, in place (tensors that already ARE the static ones are left alone)"""
    for k, v in (batch or {}).items():
        dst = static.get(k)
        if torch.is_tensor(v) and torch.is_tensor(dst) and v.data_ptr() != dst.data_ptr():
            dst.copy_(v, non_blocking=True)


def _graph_node_count(graph: "torch.cuda.CUDAGraph") -> Optional[int]:
    """Number of nodes of a captured graph (hipGraphGetNodes on the raw handle; the graph must have been created with
    keep_graph=True).  None if the runtime does not answer."""
    import ctypes
    try:
        hip = ctypes.CDLL('libamdhip64.so')
        n = ctypes.c_size_t(0)
        rc = hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n))
        return int(n.value) if rc == 0 else None
    except (OSError, AttributeError, RuntimeError):
        return None


class GraphedModuleStep:
    """``trainer.train_step(batch)`` of a trainer whose forward goes through the model's own module (directional
    and single-position models) captured into ONE HIP graph.  The batch lives in static device buffers that
    ``__call__`` refreshes in place; warm-up and capture run on one private stream (``_warm_up``).  Needs ``capturable=True``
    (flat Adam with device-side step counter and learning rates) and a loss path without host reads: with ``use_edc_mask``
    the directional trainer's time mask (reference losses.py:287-292, :355-360: drawn on the host every step) is drawn INSIDE
    the graph by the counter-based device generator (``mask_seed``; the bits of ``gfdn_draw_mask`` at (seed, replay number))."""

    graph = None

    def __init__(self, trainer, example_batch: Dict, mask_seed: Optional[int] = None):
        if not trainer.capturable:
            raise ValueError("build the trainer with capturable=True to replay steps from a graph")
        self.mask_state = None
        if trainer.config.use_edc_mask:
            crit = trainer.criterion[0]
            if not isinstance(crit, directional_edc_loss):
                raise NotImplementedError("GraphedModuleStep: a device-side EDC mask exists for the directional loss only")
            K = example_batch['z_values'].shape[-1]
            L = min(crit.edc_len_samps, 2 * (K - 1) - crit.mixing_time_samps)
            dev = example_batch['z_values'].device
            if mask_seed is None:
                mask_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.long).item())   # torch.manual_seed governs it
            self.mask_seed = int(mask_seed)
            self.mask_state = torch.zeros(1, dtype=torch.long, device=dev)
            self.maskw = torch.zeros(L, dtype=torch.float32, device=dev)
            self._crit = crit              # (the device generator is installed on the criterion around warm-up and capture
            #                                 only -- device_mask_scope --: eager steps and validation on the same trainer
            #                                 keep the host draw that torch.manual_seed governs)
        self.tr = trainer
        self.batch = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in example_batch.items()}
        self.stream = None                 # (created by capture(): torch hands streams out of a pool of 32 round-robin, and
        #                                     a DirectionalBank's steps never capture on their own)
        self.out = None

    @contextlib.contextmanager
    def device_mask_scope(self):
        """The criterion draws its EDC time mask from this step's device generator inside the block"""
        if self.mask_state is None:
            yield
            return
        prev = self._crit.device_mask
        self._crit.device_mask = (self.mask_seed, self.mask_state, self.maskw)
        try:
            yield
        finally:
            self._crit.device_mask = prev

    def _step(self):
        return self.tr.train_step(self.batch)

    def _warm_up(self, stream):
        # (the warm-up's mask draws leave no trace either)
        _warm_up(self.tr, stream, self._step, None if self.mask_state is None else self.mask_state.zero_)

    def capture(self):
        if self.stream is None:
            self.stream = torch.cuda.Stream()
        with self.device_mask_scope():
            self._warm_up(self.stream)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.stream):
                self.out = self._step()
            self._grids = _pinned_grids()
            torch.cuda.synchronize()
        return self

    def __del__(self):
        _drain_for(self.graph)

    def __call__(self, batch: Optional[Dict] = None):
        _refresh(self.batch, batch)
        if self.graph is None:
            self.capture()
        self.graph.replay()
        return self.out


class DirectionalBank:
    """The octave bands' directional trainers (reference run_subband_training_treble.py:175-204 builds one
    ``DirectionalFDNVarReceiverPosTrainer`` per band and trains them one after another) stepped TOGETHER: every band's
    ``train_step`` is captured into ONE HIP graph, the bands dealt round-robin onto ``lanes`` streams inside the capture, so
    that one replay steps all bands and one band's latency-bound stretches (the crossbar-bound 9 x 9 eliminations, a dozen
    launches of a few microseconds) run beside another band's bandwidth-bound kernels without the host launching seven
    graphs.  The bands stay independent models with their own parameters, optimiser state and loss modules -- this is a bank
    at the level of the GRAPH, not of the launch (a launch per stage for all bands would need the band dimension in every
    kernel of the directional step, as ``bandbank.BandBank`` has for the omnidirectional model).
    ``batches``: one batch dict per band; they live in static device buffers that ``__call__`` refreshes in place."""

    graph = None

    def __init__(self, trainers, example_batches, lanes: int = 2, mask_seed: Optional[int] = None):
        if len(trainers) != len(example_batches) or not trainers:
            raise ValueError("DirectionalBank: one example batch per band trainer")
        self.steps = [GraphedModuleStep(tr, b, None if mask_seed is None else mask_seed + q)
                      for q, (tr, b) in enumerate(zip(trainers, example_batches))]
        # torch hands streams out of a pool of 32 per device, round-robin: in a process that has created many, two "new"
        # streams can be the SAME stream -- a lane that aliases another lane or a band's side stream turns the fork / join
        # pattern below into one the capture rejects ("unjoined work").  Every stream of the bank is checked to be distinct.
        taken = set()

        def fresh():
            for _ in range(64):
                st = torch.cuda.Stream()
                if st.cuda_stream not in taken:
                    taken.add(st.cuda_stream)
                    return st
            raise RuntimeError("DirectionalBank: no distinct stream left in the pool")

        self.lanes = [fresh() for _ in range(max(1, min(int(lanes), len(trainers))))]
        # (the bank rearranges its trainers' streams and branches: what they had is put back by close())
        self._restore = [(tr, tr.concurrent_branches, tr._side) for tr in trainers]
        self.root = self.lanes[0]          # (the capture's origin is the first lane: the rules at _warm_up)
        for q, tr in enumerate(trainers):
            if q % len(self.lanes):
                # a band on a lane beside the first runs its colorless branch on the lane itself, not on the trainer's side
                # stream (the bands of the OTHER lanes run beside it anyway)
                tr.concurrent_branches = False
            elif tr.concurrent_branches:
                tr._side = fresh()                             # (the first lane's bands keep a side stream)
        self.out = None

    def close(self):
        """Hands the trainers back as they came: their own side streams and ``concurrent_branches`` (the captured graph keeps
        replaying on the bank's lanes; eager steps of a trainer run as before the bank was built)."""
        for tr, branches, side in self._restore:
            tr.concurrent_branches, tr._side = branches, side
        self._restore = []

    @property
    def batches(self):
        return [st.batch for st in self.steps]

    def _lane(self, q: int):
        return self.lanes[q % len(self.lanes)]

    def render(self, z_values, norm_listener_position, taps, length: int, directional: bool = True, rows=None, out=None,
               chunk: int = 4096):
        """The spatial RIRs of all receivers from the bank's bands as they stand (``subband.infer_directional_bands`` on
        the trainers' nets, band q filtered with ``taps[q]``): (len(rows) or R, J or (order+1)^2, length) float32."""
        from .subband import infer_directional_bands
        return infer_directional_bands([st.tr.net for st in self.steps], z_values, norm_listener_position, taps, length,
                                       directional=directional, rows=rows, out=out, chunk=chunk)

    def render_binaural(self, z_values, norm_listener_position, taps, length: int, hrir_sh, path, rotations, stimulus,
                        update_ms: float = 100.0, alpha: float = 0.5, fade_len_ms: Optional[float] = None,
                        sample_rate: Optional[float] = None, chunk: int = 32, out=None):
        """A dry stimulus heard binaurally by a listener who moves along ``path`` and turns their head, from the bank's
        bands as they stand (``subband.render_binaural_moving_listener_bands`` on the trainers' nets): (P h, 2) float32."""
        from .subband import render_binaural_moving_listener_bands
        return render_binaural_moving_listener_bands([st.tr.net for st in self.steps], z_values, norm_listener_position, taps,
                                                     length, hrir_sh, path, rotations, stimulus, update_ms=update_ms,
                                                     alpha=alpha, fade_len_ms=fade_len_ms, sample_rate=sample_rate,
                                                     chunk=chunk, out=out)

    def capture(self):
        with contextlib.ExitStack() as scopes:
            for st in self.steps:
                scopes.enter_context(st.device_mask_scope())
            for q, st in enumerate(self.steps):
                st._warm_up(self._lane(q))
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            outs = [None] * len(self.steps)
            with torch.cuda.graph(self.graph, stream=self.root):
                for lane in self.lanes[1:]:
                    lane.wait_stream(self.root)                    # fork
                for q, st in enumerate(self.steps):
                    with torch.cuda.stream(self._lane(q)):
                        outs[q] = st._step()
                for lane in self.lanes[1:]:
                    self.root.wait_stream(lane)                    # join
            self.out = outs
            self._grids = _pinned_grids()
            torch.cuda.synchronize()
        return self

    def __del__(self):
        _drain_for(self.graph)

    def __call__(self, batches=None):
        for st, batch in zip(self.steps, batches or ()):
            _refresh(st.batch, batch)
        if self.graph is None:
            self.capture()
        self.graph.replay()
        return self.out


class GraphedTrainStep:
    """One optimiser step (collate -> normalize -> forward -> losses -> backward -> [all-reduce] ->
    Adam) captured into HIP graphs and replayed: ~400 kernel launches per step collapse into one
    (two with the RCCL all-reduce of the flat gradient buffer between them) graph launch, which removes the host launch
    overhead that dominates the eager step (profiles/).

    Per step the host only writes one static device buffer, the receiver indices of the batch.
    The EDC time mask (losses.py:221-223) is drawn INSIDE the graph by a counter-based device
    generator (``mask_source='device'``, the default): the CPU draw costs ~0.5 ms per step on the
    host, which is as long as the whole GPU step, and in a data-parallel job every rank derives
    the same mask from the shared seed with no broadcast.  ``mask_source='host'`` keeps the
    reference's CPU draw (uniform_ then bernoulli from torch's global generator), staged through
    pinned memory.  Requires a fixed batch size.

    What a trainer offers to be graphed (``VarReceiverPosTrainer`` and ``bandbank.BandBankTrainer`` do):
      ``capturable`` (True), ``net``, ``optimizer`` (a ``FlatAdam``), ``criterion[1]`` (the EDC loss), ``stft_win``;
      ``num_bands`` (models stepped at once; above 1 the loss heads are (bands,) vectors), ``_decay_window(K)`` (start and
      length of the longest EDC window), ``_target_window(K)`` (for ``dataset.precompute_decay_targets``) and
      ``_item_windows(K, Bper, device)`` ((None, None) where one window serves all bands, else also ``_band_mask_rows``);
      ``_step_losses(batch, mask_prenorm=, normalize_first=, defer_total=)``, the forward and losses under autograd, or
      ``_fused``, a ``bankstep.FusedBankStep`` in its place (None: autograd; with it ``_stream(name)`` and a bank as ``net``);
      ``world_size``, ``rank``, ``process_group``, ``_allreduce`` (None: one process) and ``allreduce_in_graph`` (whether to
      try capturing the collective inside the step's one graph)."""

    graph_a = graph_b = graph_p = None
    # steps per graph of the pipelined chain (even; 0: single-step graphs only).  OFF by default: measured on the 7-band
    # step, same box, 400 steps: 0.681 ms single-step graphs, 0.692 / 0.688 / 0.688 ms with 2 / 4 / 8 steps per graph.
    # Under rocprofv3 the interior steps of a chain are 35 us shorter (no wait for the gains at the head, Adam straight
    # behind the last gradient kernel, no join), but the chain's last step waits for the side stream's run-ahead work
    # (+60 us per graph) and without the profiler's per-kernel serialisation the interior gain is not there either.
    pipe_steps = 0

    def __init__(self, trainer, dataset, batch_size: int, mask_source: str = "device", mask_seed: Optional[int] = None):
        if not trainer.capturable:
            raise ValueError("build the trainer with capturable=True to replay steps from a graph")
        if mask_source not in ("device", "host"):
            raise ValueError("mask_source must be 'device' or 'host'")
        self.tr, self.ds, self.B = trainer, dataset, batch_size
        self.mask_source = mask_source
        dev = dataset.device
        K = dataset.rir_mag_response.shape[-1]
        self.start, self.length = trainer._decay_window(K)
        # a band bank (bandbank.BandBankTrainer) steps ``num_bands`` independent models at once: the
        # batch holds batch_size / num_bands receivers per model, and loss heads are (bands,) vectors
        self.num_bands = trainer.num_bands
        if batch_size % self.num_bands:
            raise ValueError("batch size must be a multiple of the number of bands")
        self.gb = batch_size // self.num_bands * trainer.world_size
        # replayed launches read the targets through the static index buffer: they must come from
        # the dataset-level store (a by-pointer cache would go stale under replay).  A band bank whose bands have
        # different EDC windows keeps targets of per-band lengths and one row of mask weights per band
        dataset.precompute_decay_targets(trainer.stft_win, *trainer._target_window(K))   # (no-op when the stores hold them)
        _, self.band_len = trainer._item_windows(K, batch_size // self.num_bands, dev)
        self.idx = torch.zeros(batch_size, dtype=torch.long, device=dev)
        if self.band_len is None:
            self.maskw = torch.full((self.length,), 1.0 / (self.gb * self.length), dtype=torch.float32, device=dev)
        else:
            self.maskw = trainer._band_mask_rows(None, K, self.gb, dev)          # (bands, length): no mask = all kept
        self._K = K
        # ring of pinned staging buffers: the async H2D copy of step i is only executed when the
        # stream reaches it, so its source must not be rewritten by the host preparing step i+1
        self._ring = [(torch.empty(self.length, dtype=torch.float32).pin_memory(),
                       torch.empty(batch_size, dtype=torch.long).pin_memory(), torch.cuda.Event())
                      for _ in range(4)]
        self._ring_pos = 0
        self.mask_state = torch.zeros(1, dtype=torch.long, device=dev)     # draws made so far
        self._one = torch.ones(() if self.num_bands == 1 else (self.num_bands,), dtype=torch.float32,
                               device=dev)                                  # root gradient of the heads
        if mask_seed is None:
            seed_t = torch.randint(0, 2 ** 62, (1,), dtype=torch.long)      # torch.manual_seed governs it
            if trainer.world_size > 1:                                      # one seed for all ranks, once
                seed_t = seed_t.to(dev)
                dist.broadcast(seed_t, src=0, group=trainer.process_group)
            mask_seed = int(seed_t.item())
        self.mask_seed = int(mask_seed)
        self._tail_in_graph = False
        self.collective_probe_nodes = None        # nodes the probe's captured all-reduce left in its graph (None: no probe)
        self.losses = None
        # receiver schedule (load_schedule / run_next): the batches of an epoch live on the device and every step ends
        # by fetching the next step's receivers into ``idx`` -- no host copy in front of a replay
        self.sched_cap = 1024
        self.sched = torch.zeros((self.sched_cap, batch_size), dtype=torch.long, device=dev)
        self.sched_state = torch.tensor([0, 1], dtype=torch.long, device=dev)        # {position, length}

    @property
    def _mask_drawn_on(self) -> Optional[str]:
        """'device' / 'host': who draws the EDC time mask of a step; None: the loss takes every index"""
        return self.mask_source if self.tr.criterion[1].use_mask else None

    def _ensure_records(self):
        """The explicit bank step's graph starts from the records its previous replay left (bankstep.FusedBankStep): if
        anything else has touched the parameters since, rebuild them in front of the replay."""
        fused = self.tr._fused
        if fused is None:
            return
        if self._tail_in_graph:
            fused.ensure_records()
        else:
            fused.invalidate_records()        # (this graph evaluates its own records and leaves the parameters changed)

    # -- receiver schedule --------------------------------------------------------------------
    def _pick_next(self):
        ops.pick_rows(self.sched, self.sched_state, self.idx)

    def load_schedule(self, batches):
        """Upload the receivers of the next ``len(batches)`` steps (each ``batch_size`` dataset rows; at most
        ``sched_cap`` steps) and point the step at the first of them; ``run_next()`` then replays one step per call.
        The reference's DataLoader likewise fixes an epoch's batches when the epoch starts (trainer.py:373-379)."""
        # (a (steps, batch) int64 tensor -- pinned host memory for an asynchronous upload -- is taken as it is; lists of indices
        # are converted here, which costs ~0.2 ms for 20 x 224 Python integers.  A PINNED source is read by the copy engine
        # AFTER this call returns: the caller must leave it unmodified until the current stream has passed this point -- an
        # event is kept in ``sched_uploaded`` for callers that refill one pinned table)
        t = batches.to(torch.long) if torch.is_tensor(batches) else torch.as_tensor([list(b) for b in batches], dtype=torch.long)
        n = t.shape[0]
        if n == 0 or n > self.sched_cap or t.shape[1] != self.B:
            raise ValueError(f"load_schedule: 1..{self.sched_cap} batches of {self.B} receivers")
        self.sched[:n].copy_(t, non_blocking=True)
        self.sched_uploaded = torch.cuda.Event()
        self.sched_uploaded.record()
        self.sched_state.copy_(torch.tensor([0, n], dtype=torch.long))
        self._pick_next()                                 # idx <- first batch, position 1
        return n

    def _replay(self, indices):
        if self.graph_a is None:
            self.capture(indices)
        self._load_inputs(indices)
        self._ensure_records()
        self.graph_a.replay()
        if self.graph_b is not None:
            self.tr._allreduce()
            self.graph_b.replay()
        return self.losses

    def __call__(self, indices):
        """Run one optimiser step on the receivers ``indices``; returns the static loss tensors
        (valid until the next call)."""
        return self._replay(indices)

    def run_next(self):
        """One optimiser step on the next batch of the loaded schedule (wraps around at its end); returns the static
        loss tensors (valid until the next step)."""
        return self._replay(None)

    def run_schedule(self, batches):
        """Generator over the steps of ``batches`` (any number: uploaded in chunks of ``sched_cap``).  Where the
        pipelined chain applies (:meth:`_pipe_ok`) the steps run ``pipe_steps`` at a time from one graph and the rest
        from the single-step graph -- same numbers either way."""
        if not torch.is_tensor(batches):
            batches = list(batches)
        for i0 in range(0, len(batches), self.sched_cap):
            n = self.load_schedule(batches[i0:i0 + self.sched_cap])
            done = 0
            S = self.pipe_steps
            if self._pipe_ok() and n >= S:
                if self.graph_p is None:
                    self.capture_pipe()
                self._pipe_prologue()
                while n - done >= S:
                    self.graph_p.replay()
                    self.tr._fused.invalidate_records()      # (the chain evaluates its own records: the kept ones are stale)
                    for losses in self.pipe_losses:
                        yield losses
                    done += S
            for _ in range(n - done):
                yield self.run_next()

    # -- pipelined chain of explicit bank steps (bankstep.StepPipe; ``pipe_steps`` above) ---------
    def _pipe_ok(self) -> bool:
        tr = self.tr
        return (self.pipe_steps >= 2 and self.pipe_steps % 2 == 0 and tr._fused is not None
                and tr._allreduce is None and tr._stream('_side2') is not None and self._mask_drawn_on != "host")

    def _mlp_args(self):
        bank = self.tr.net
        Hh, n_hidden, _, lo, hi = bank._mlp_cfg
        return (self.ds.norm_listener_position, bank._freq_pi, bank.output_scalars_w.detach(), Hh, n_hidden,
                bank.num_groups, lo, hi, self.idx, self.num_bands)

    def _pipe_prologue(self):
        """Receiver gains of the batch in ``idx`` at the current parameters -> the chain's first buffer set."""
        ops.mlp_gains_fwd(*self._mlp_args(), out=self._pipe_bufs[0])

    def capture_pipe(self):
        """Record ``pipe_steps`` explicit steps as ONE graph with the side stream running ahead (StepPipe)."""
        if self.graph_a is None:
            self.capture(None)                      # (warm-up of every kernel, lazy initialisations)
        bank = self.tr.net
        Hh, n_hidden = bank._mlp_cfg[0], bank._mlp_cfg[1]
        if bank.mixed_networks:
            raise NotImplementedError("a pipelined chain of steps takes a bank of equal gain networks")
        dev, G, nl = self.idx.device, bank.num_groups, 1 + n_hidden
        mk = lambda: (torch.empty((self.B, G), dtype=torch.float32, device=dev),
                      torch.empty((self.B, nl, Hh), dtype=torch.float32, device=dev),
                      torch.empty((self.B, nl), dtype=torch.float32, device=dev))
        self._pipe_bufs = [mk(), mk()]
        pipe = StepPipe(self._pipe_bufs, self.pipe_steps)
        rng_state = torch.get_rng_state()
        torch.cuda.synchronize()
        self.graph_p = torch.cuda.CUDAGraph()
        losses = []
        with torch.cuda.graph(self.graph_p, stream=self._capture_stream):
            for _ in range(self.pipe_steps):
                losses.append(dict(self._fused_fwd_bwd(opt_step=True, pipe=pipe)))
        self.pipe_losses = losses
        self._grids = _pinned_grids()
        torch.set_rng_state(rng_state)
        return self

    # -- pieces -------------------------------------------------------------------------------
    def _draw_device_mask(self):
        """``maskw`` <- the mask of draw number ``mask_state`` (which it advances), pre-divided by the global batch"""
        ops.draw_mask(self.mask_seed, self.mask_state, self.length, 1.0 / self.gb, out=self.maskw, band_len=self.band_len)

    def _fwd_bwd(self):
        tr = self.tr
        if self._mask_drawn_on == "device":
            # (measured: drawing it on the EDC side stream adds a third branch at the head of the graph
            # and the executor then serialises the whole front: +0.05 ms)
            self._draw_device_mask()
        # no gather: the kernels read the dataset-level stores through the static index buffer
        batch = self.ds.collate(self.idx, lean="rows")
        tr.optimizer.zero_grad(set_to_none=True)
        losses = tr._step_losses(batch, mask_prenorm=self.maskw, normalize_first=True, defer_total=True)
        heads = losses.pop('_heads')
        torch.autograd.backward(heads, [self._one] * len(heads))      # no ones-fill, no add in front
        with torch.no_grad():
            losses['_total'] = heads[0].detach() if len(heads) == 1 else heads[0].detach() + heads[1].detach()
        return losses

    def _fused_fwd_bwd(self, opt_step: bool, pipe=None):
        """The band bank's explicit launch sequence (bankstep.FusedBankStep): mask draw, normalize, forward, losses,
        backward into the flat gradient buffer [, all-reduce, Adam]."""
        tr = self.tr
        batch = self.ds.collate(self.idx, lean="rows")
        return tr._fused.run(batch, self.maskw, 1.0, normalize_first=True, train=True, allreduce=tr._allreduce,
                             opt_step=opt_step, tail=self._pick_next, pipe=pipe,
                             mask_draw=self._draw_device_mask if self._mask_drawn_on == "device" else None)

    # one graph records _eager(); two graphs around an eager collective record _until_collective() and _after_collective()
    def _until_collective(self):
        """Forward, losses, backward and the gradients in the flat bucket: everything in front of the all-reduce"""
        if self.tr._fused is not None:
            return self._fused_fwd_bwd(opt_step=False)
        losses = self._fwd_bwd()
        self.tr.optimizer.pack_grads()
        return losses

    def _after_collective(self):
        """Adam on the reduced gradients and the next step's receivers: everything behind the all-reduce"""
        if self.tr._fused is not None:
            # (the collective itself runs between the replays)
            self._apply_reduced(self.tr._fused.finish(lambda: None))
        else:
            self.tr.optimizer.step()
            self._pick_next()

    def _eager(self):
        if self.tr._fused is not None:
            return self._fused_fwd_bwd(opt_step=True)      # (the explicit step issues collective, Adam and tail itself)
        losses = self._until_collective()
        if self.tr._allreduce is not None:
            self.tr._allreduce()
        self._after_collective()
        return losses

    # -- capture ------------------------------------------------------------------------------
    def capture(self, indices):
        """Warm up (``_warm_up``: eagerly, on the private stream of the capture, leaving no trace), then record the graphs."""
        tr = self.tr
        rng_state = torch.get_rng_state()                  # capture is RNG-neutral
        self._load_inputs(indices)
        saved_sched = (self.sched_state.clone(), self.idx.clone())     # (the warm-up steps advance the schedule)

        def also_reset():
            self.mask_state.zero_()
            self.sched_state.copy_(saved_sched[0])
            self.idx.copy_(saved_sched[1])
            if tr._fused is not None:
                # the explicit step keeps the records of the current parameters between steps (its fused tail leaves the
                # next step's): those of the restored parameters, so that the capture holds no records launch
                tr._fused.prime_records()

        side = self._capture_stream = torch.cuda.Stream()
        _warm_up(tr, side, self._eager, also_reset)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # One step structure for the WHOLE group: every rank probes for itself (the probe never raises), then the
        # verdicts are reduced with MIN -- a rank that cannot capture the collective takes every other rank with it to
        # the two-graph step, so no two ranks ever pair a captured all-reduce with an eager one (a hang)
        in_graph = False
        if tr._allreduce is not None and tr.allreduce_in_graph:
            in_graph = self._all_ranks_agree(self._collective_is_capturable())
        self.allreduce_in_graph = in_graph
        self.graph_a = torch.cuda.CUDAGraph()
        if tr._allreduce is None or in_graph:
            # ONE graph: forward, backward, [all-reduce of the gradient bucket (RCCL is capturable),] Adam
            with torch.cuda.graph(self.graph_a, stream=side):
                self.losses = self._eager()
        else:
            # forward + backward + pack | all-reduce of the gradient bucket (eager RCCL) | Adam
            with torch.cuda.graph(self.graph_a, stream=side):
                self.losses = self._until_collective()
            self.graph_b = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_b, pool=self.graph_a.pool(), stream=side):
                self._after_collective()
        self.losses = dict(self.losses)
        # whether the captured step ends by leaving the next step's records (bankstep.FusedBankStep: fused tail) -- such a
        # graph holds no records launch and relies on _ensure_records() in front of every replay
        self._tail_in_graph = bool(tr._fused is not None and tr._fused._rec_valid)
        self._grids = _pinned_grids()
        torch.set_rng_state(rng_state)
        return self

    def __del__(self):
        _drain_for(self.graph_a, self.graph_p)

    def _apply_reduced(self, red):
        """Split-graph data-parallel step: the second graph rebuilt the decay losses from the reduced slots."""
        if red is None:
            return
        sums, total = red
        nb = self.num_bands
        self.losses = dict(self.losses)
        self.losses['edr_loss'] = sums[:, 1] if nb > 1 else sums[1]
        self.losses['edc_loss'] = sums[:, 2] if nb > 1 else sums[2]
        self.losses['_total'] = total

    def _all_ranks_agree(self, ok: bool) -> bool:
        """MIN of the ranks' verdicts (one small collective, issued by every rank whatever its own verdict)."""
        tr, pg = self.tr, self.tr.process_group
        if not dist.is_initialized() or dist.get_world_size(pg) == 1:
            return bool(ok)
        on_host = dist.get_backend(pg) != 'nccl'
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, device='cpu' if on_host else self.idx.device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=pg)
        agreed = bool(int(t.item()))
        if ok and not agreed and tr.rank == 0:
            print("[diffgfdn_amd] another rank cannot capture the all-reduce: two-graph step on every rank")
        return agreed

    def _collective_is_capturable(self) -> bool:
        """Probe: capture the trainer's collective on a scratch tensor in a throw-away graph and replay it.  Any
        error -> the step falls back to two graphs with the collective between them (the same result)."""
        tr, pg = self.tr, self.tr.process_group
        if not dist.is_initialized() or dist.get_backend(pg) != 'nccl':
            return False               # (gloo rehearsals: host-side collectives cannot be captured)
        try:
            probe = torch.ones(64, dtype=torch.float32, device=self.idx.device)
            dist.all_reduce(probe, group=pg)                     # communicator set up outside the capture
            torch.cuda.synchronize()
            probe.fill_(1.0)
            g = torch.cuda.CUDAGraph(keep_graph=True)
            with torch.cuda.graph(g):
                dist.all_reduce(probe, group=pg)
            # how many nodes the captured collective left in the graph (0 on a one-rank group, where the library
            # makes an in-place all-reduce a no-op: such a probe says nothing about capturing a collective)
            self.collective_probe_nodes = _graph_node_count(g)
            g.replay()
            torch.cuda.synchronize()
            ok = bool((probe == float(dist.get_world_size(pg))).all().item())
            del g
            return ok
        except Exception as e:                                   # noqa: BLE001 -- any failure means "do not capture"
            if tr.rank == 0:
                print(f"[diffgfdn_amd] all-reduce not capturable here ({type(e).__name__}: {e}); two-graph step")
            torch.cuda.synchronize()
            return False

    def _load_inputs(self, indices):
        tr = self.tr
        host_mask, host_idx, ev = self._ring[self._ring_pos]
        self._ring_pos = (self._ring_pos + 1) % len(self._ring)
        host_draw = self._mask_drawn_on == "host"
        if indices is None and not host_draw:
            return                           # schedule mode: the previous step (or load_schedule) has filled idx
        ev.synchronize()                     # the copies that last used this slot have executed
        if indices is not None:
            host_idx.copy_(torch.as_tensor(list(indices), dtype=torch.long))
            self.idx.copy_(host_idx, non_blocking=True)
        if host_draw:
            keep = torch.bernoulli(torch.empty(self.length).uniform_(0, 1))
            if tr.world_size > 1:
                # one mask for all ranks: rank 0's draw wins
                keep = keep.to(self.maskw.device)
                dist.broadcast(keep, src=0, group=tr.process_group)
            if self.band_len is not None:
                # bands with different windows: one draw of the longest, truncated per band (as the device draw)
                self.maskw.copy_(tr._band_mask_rows(keep, self._K, self.gb, self.maskw.device))
            elif tr.world_size > 1:
                self.maskw.copy_(keep / (keep.sum() * self.gb))
            else:
                # (one process: normalised on the host into pinned memory and copied asynchronously -- no host sync)
                torch.div(keep, float(keep.sum()) * self.gb, out=host_mask)
                self.maskw.copy_(host_mask, non_blocking=True)
        ev.record()
