"""Host-side launch order of the band bank's explicit step (diffgfdn_amd/bankstep.py), pinned to a recorded fixture.

The step's speed is decided by the order in which launches and cross-stream edges are issued from the host (DESIGN.md
section 5); the numeric tests would not notice a launch that moved to another stream or a wait that moved in front of a
launch.  A recorder, active while one step is issued, logs in host order
  ["launch", entry point, stream]      every call into the library whose prototype in include/diffgfdn_hip.h ends in the
                                       stream parameter (size queries take none and are left out),
  ["record" | "wait_event", stream, n] every torch.cuda.Event.record / Stream.wait_event (n: event number by first appearance),
  ["wait_stream", stream, other]       every Stream.wait_stream,
  ["graph_nodes", n]                   the node count of each captured graph (catches ATen launches the wrapper does not see),
with streams tagged main / side / side2.  tests/golden/bankstep_launch_order.json holds the recorded result of every case; a
change of the launch chain regenerates it deliberately (BANKSTEP_ORDER_RECORD=<file> writes the logs there) and shows the
diff.

Cases o, p and q pin the captures that the explicit step does not reach (diffgfdn_amd/graphstep.py): a classic trainer's and a
coupled bank's step under autograd (GraphedTrainStep) and a DirectionalBank on two lanes.  Their streams belong to several
objects, so the capture's own stream is "main" and every other one is s1, s2, ... by first appearance, as events are
numbered.  They were recorded on 92b97af, before these classes moved out of trainer.py, by
  BANKSTEP_ORDER_RECORD=<file> pytest tests/test_gpu_bankstep_order.py -k "o_ or p_ or q_"
and merged into the fixture."""
import contextlib
import json
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bankstep_launch_order.json")
FORMS4 = ("edc_one_launch", "scale_late", "fused_tail")
# case -> (bank, receivers per band, what is recorded, switches set to False)
CASES = {
    "a_defaults": ("full", 2, "capture", ()),
    "b_four_per_band": ("full", 4, "capture", ()),
    "c_valid_step": ("full", 2, "valid", ()),
    "d_no_linear_transforms": ("full", 2, "capture", ("linear_transforms",)),
    "e_no_spectral_edr": ("full", 2, "capture", ("spectral_edr",)),
    "f_small_grid": ("small", 4, "capture", ()),
    "g_pipelined_chain": ("small", 4, "pipe", ("linear_transforms",)),
    "h_round4_forms": ("full", 2, "capture", FORMS4),
    "i_no_fused_tail": ("full", 2, "capture", ("fused_tail",)),
    "j_eight_lines": ("full8", 4, "capture", ()),
    "k_eight_lines_matrix_cores": ("full8", 4, "capture", ("transform_polys",)),
    "l_split_data_parallel": ("small", 4, "split", ()),
    # (the normalisation scale inside the receiver gains needs the wave-per-receiver gain network: 8 receivers per band)
    "m_gain_fold": ("full", 8, "capture", ()),
    "n_gain_fold_eight_lines": ("full8", 8, "capture", ()),
    # captures outside the explicit step: (what is captured, -, "graph", -)
    "o_classic_trainer": ("classic", None, "graph", ()),                 # N = 16, K = 4 097, 4 receivers, STFT window 512
    "p_coupled_bank": ("coupled", None, "graph", ()),                    # 3 bands, G = 3, 4 receivers per band
    "q_directional_bank_two_lanes": ("directional", None, "graph", ()),  # 3 bands on 2 lanes, device-side EDC masks
}


def _launching_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "diffgfdn_hip.h")).read(), flags=re.S)
    protos = re.finditer(r"\b(gfdn_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text)
    return {m.group(1) for m in protos if re.search(r"\bstream\s*$", m.group(2))}


@contextlib.contextmanager
def _recording(tr, capturing_only=True):
    """Yields the log; ``capturing_only``: entries are taken between capture_begin and capture_end only (the warm-up steps
    in front of a capture are not part of the replayed order).  ``tr`` None: streams are tagged by first appearance."""
    from diffgfdn_amd import _lib
    from diffgfdn_amd.trainer import _graph_node_count
    log, events, others, state = [], [], [], {"capturing": 0, "nested": 0, "origin": None}
    launching, real = _launching_entry_points(), _lib.load()

    def tag(stream):
        if tr is not None:
            return next((w[1:] for w in ("_side", "_side2") if stream == tr._stream(w)), "main")
        if stream == state["origin"]:
            return "main"
        if stream not in others:
            others.append(stream)
        return f"s{others.index(stream) + 1}"

    def add(*entry):
        if not state["nested"] and (state["capturing"] or not capturing_only):
            log.append([number(e) if isinstance(e, torch.cuda.Event) else tag(e) if isinstance(e, torch.cuda.Stream) else e
                        for e in entry])

    def number(ev):
        if not any(e is ev for e in events):
            events.append(ev)
        return next(i for i, e in enumerate(events) if e is ev)

    class Lib:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in launching:
                return fn
            return lambda *a: (add("launch", name, torch.cuda.current_stream()), fn(*a))[1]

    class Graph(torch.cuda.CUDAGraph):
        def capture_begin(self, *a, **kw):
            super().capture_begin(*a, **kw)
            state["origin"] = state["origin"] or torch.cuda.current_stream()
            state["capturing"] += 1

        def capture_end(self):
            super().capture_end()
            nodes = _graph_node_count(self)
            if nodes is not None:
                add("graph_nodes", nodes)
            state["capturing"] -= 1

    orig = (torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream, torch.cuda.CUDAGraph)

    def record(ev, stream=None):
        add("record", torch.cuda.current_stream() if stream is None else stream, ev)
        orig[0](ev, stream)

    def wait_event(stream, ev):
        add("wait_event", stream, ev)
        orig[1](stream, ev)

    def wait_stream(stream, other):
        add("wait_stream", stream, other)
        state["nested"] += 1                  # (its own record + wait_event are not entries)
        try:
            orig[2](stream, other)
        finally:
            state["nested"] -= 1

    torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream = record, wait_event, wait_stream
    torch.cuda.CUDAGraph, _lib._lib = (lambda keep_graph=False: Graph(keep_graph=True)), Lib()
    try:
        yield log
    finally:
        torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream, torch.cuda.CUDAGraph = orig
        _lib._lib = real


def _bank(kind):
    """(trainer, stacked dataset, rows of the captured batch per receivers-per-band)"""
    from diffgfdn_amd.bandbank import BandBank, BandBankTrainer, BandStackedDataset
    if kind == "small":
        from tests import test_gpu_bank as gb
        _, _, _, _, tr, sds, _ = gb._bank_setup(mask=True)
        return tr, sds, {4: [[0, 3, 5, 7], [1, 2, 8, 11], [4, 6, 9, 10]]}
    from tests import test_gpu_fullsize as fs
    bands = [fs._band(q, delays=[d + 2 * q for d in fs.DELAYS32] if kind == "full8" else None) for q in range(2)]
    filt = torch.tensor(fs._filters(), device="cuda").to(torch.complex64)
    tr = BandBankTrainer(BandBank([b_[2] for b_ in bands]), fs._tc(), subband_filter_freq_resp=filt, band_names=fs.CENTRES)
    return tr, BandStackedDataset([b_[1] for b_ in bands]), {2: [[0, 3], [1, 4]], 4: [[0, 3, 1, 5], [1, 4, 2, 0]],
                                                                8: [[0, 3, 1, 5, 2, 4, 0, 3], [1, 4, 2, 0, 5, 3, 1, 4]]}


def _record_graph_case(kind):
    """One capture of a tiny model through the classes of diffgfdn_amd/graphstep.py, set up as the parity tests do"""
    import warnings
    from diffgfdn_amd.trainer import DirectionalBank, VarReceiverPosTrainer
    from tests import test_gpu_bank_coupled as gc
    from tests import test_gpu_parity as gp
    if kind == "classic":
        fx, ds, tc = gp._graphed_step_setup()
        tr = VarReceiverPosTrainer(gp._grid_model(fx), tc, stft_win=512, capturable=True)
        capture = tr.graphed(ds, 4, mask_seed=4242).capture, ([0, 1, 2, 3],)
    elif kind == "coupled":
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message="BandBankTrainer: this layout", category=RuntimeWarning)
            _, _, _, _, tr, sds, _ = gc._bank_setup(3)
        assert tr._fused is None
        capture = tr.graphed(sds, gc.NPER, mask_seed=777).capture, (sds.global_rows(gc.SELS),)
    else:
        capture = DirectionalBank(*gp._directional_bands(mask=True), lanes=2, mask_seed=977).capture, ()
    with _recording(None) as log:
        capture[0](*capture[1])
    torch.cuda.synchronize()
    assert sum(e[0] == "launch" for e in log) >= 8 and sum(e[0] == "graph_nodes" for e in log) == 1, log
    return log


def _record_case(case):
    kind, per, what, off = CASES[case]
    if what == "graph":
        return _record_graph_case(kind)
    tr, sds, sels = _bank(kind)
    assert tr._fused is not None
    for name in off:
        assert getattr(tr._fused, name) is True
        setattr(tr._fused, name, False)
    rows = sds.global_rows(sels[per])
    if what == "split":
        tr._allreduce = lambda: None
    step = tr.graphed(sds, per, mask_seed=5)
    if what == "valid":
        step.capture(rows)
        torch.manual_seed(5)                          # (the validation step draws its EDC mask on the host)
        tr.valid_step(sds.collate(rows))              # (tables and dataset-level stores built)
        with _recording(tr, capturing_only=False) as log:
            tr.valid_step(sds.collate(rows))
    elif what == "pipe":
        step.pipe_steps = 2
        assert step._pipe_ok()
        step.load_schedule([rows, rows])
        step.capture(None)                            # (the single-step graph: capture_pipe's warm-up)
        with _recording(tr) as log:
            step.capture_pipe()
    else:
        with _recording(tr) as log:
            step.capture(rows)
        assert (step.graph_b is not None) == (what == "split")
    torch.cuda.synchronize()
    assert sum(e[0] == "launch" for e in log) >= 8, log
    return log


def _dump(logs):
    body = ",\n".join(f' "{k}": [\n' + ",\n".join("  " + json.dumps(e) for e in v) + "\n ]" for k, v in sorted(logs.items()))
    return "{\n" + body + "\n}\n"


@pytest.mark.parametrize("case", sorted(CASES))
def test_bankstep_host_launch_order(case):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    log = _record_case(case)
    out = os.environ.get("BANKSTEP_ORDER_RECORD")
    if out:
        logs = json.load(open(out)) if os.path.exists(out) else {}
        logs[case] = log
        with open(out, "w") as f:
            f.write(_dump(logs))
        return
    want = json.load(open(FIXTURE))[case]
    if log != want:
        i = next((j for j, (a, b) in enumerate(zip(log, want)) if a != b), min(len(log), len(want)))
        lines = [f"{'->' if j == i else '  '} {j:3d}  got {log[j] if j < len(log) else '(end)'}   "
                 f"recorded {want[j] if j < len(want) else '(end)'}" for j in range(max(i - 3, 0), i + 4)]
        pytest.fail(f"{case}: host order differs from the recorded one at entry {i} ({len(log)} entries against "
                    f"{len(want)})\n" + "\n".join(lines))
