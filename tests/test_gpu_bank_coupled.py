"""Band bank with learnable inter-group coupling (run_subband_training_treble.py --allow_coupling) on the MI355X.

The set-up of tests/test_gpu_bank.py (fs 8000, nfft 8192, STFT window 512, 3 bands, 12 receivers, 4 per band and step,
the same filters and synthetic rooms) with ``use_zero_coupling=False``: every band's feedback matrix is the dense
A = block_M o kron(Phi(alpha), 1), built for all bands by one launch (csrc/coupling.hip) and solved per bin with the bands
as blocks of N lines -- N = 12 (G = 3: the packed three-rows-per-lane elimination) and N = 16 (G = 4: the headline shape).

Parity chain: one bank step against every band's own VarReceiverPosTrainer step and against the CPU oracle of the reference
step with learnable angles; the graph-replayed step against the eager one; train() with checkpoints that load back into
fresh coupled modules.

Bank against the band's own trainer: the bank builds A with its own kernel (float64 inside, rounded once) where the band's
trainer runs torch's float32 einsum / kron, so the two agree to rounding, not to the bit.  Measured on an MI355X (largest
value over the bands; G = 3 / G = 4): losses 3.37e-6 / 1.31e-6 relative, post-Adam state 1.86e-7 / 1.86e-7 relative; the
bounds are three times the larger figure, far inside the oracle bounds (1e-4)."""
import numpy as np
import pytest
import torch

from tests.helpers import philox_mask, rel_err
from tests.margins import within
from tests.test_gpu_bank import BANDS, FS, NFFT, WIN, _band_filters, _tc

pytestmark = pytest.mark.gpu
DEV = "cuda"
NPER = 4
SELS = [[0, 3, 5, 7], [1, 2, 8, 11], [4, 6, 9, 10]]
# bank step against the band's own trainer step, largest value over bands and shapes, measured on an MI355X
BAND_LOSS_MEASURED, BAND_STATE_MEASURED = 3.369e-6, 1.863e-7
BAND_LOSS_BOUND, BAND_STATE_BOUND = 3 * BAND_LOSS_MEASURED, 3 * BAND_STATE_MEASURED


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(autouse=True)
def _expected_fallback_warning():
    import warnings
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="BandBankTrainer: this layout", category=RuntimeWarning)
        yield


def _delays(q, G):
    base = [173, 181, 191, 193, 197, 199, 211, 223, 227, 229, 233, 401, 239, 241, 251, 257]
    return [d + 2 * q for d in base[:G * NPER]]


def _build_net(q, G, coupling="coupled"):
    from diffgfdn_amd.config import CouplingMatrixType, FeedbackLoopConfig, OutputFilterConfig
    from diffgfdn_amd.model import DiffGFDNVarReceiverPos
    torch.manual_seed(100 + q)
    if coupling == "filter":
        fl = FeedbackLoopConfig(coupling_matrix_type=CouplingMatrixType.FILTER, pu_matrix_order=4)
    else:
        fl = FeedbackLoopConfig(coupling_matrix_type=CouplingMatrixType.SCALAR, use_zero_coupling=coupling == "zero")
    of = OutputFilterConfig(use_svfs=False, num_hidden_layers=2, num_neurons_per_layer=16, num_fourier_features=4)
    T60 = np.linspace(0.2, 0.5, G)[None, :]
    return DiffGFDNVarReceiverPos(FS, G, _delays(q, G), DEV, fl, of, use_absorption_filters=False,
                                  common_decay_times=T60, use_colorless_loss=True).to(DEV)


def _build_data(q, G, R=12):
    from diffgfdn_amd.dataloader import MultiRIRDataset, RoomDataset
    from diffgfdn_amd.synthetic import synthetic_room
    room = synthetic_room(R, G, FS, 5000, seed=10 + q, t60_range=(0.2, 0.5))
    return MultiRIRDataset(DEV, RoomDataset(G, FS, room["source_position"], room["receiver_position"],
                                            room["rirs"].copy(), room["common_decay_times"], nfft=NFFT, device=DEV))


def _bank_setup(G, coupling="coupled", R=12, **tc):
    from diffgfdn_amd.bandbank import BandBank, BandBankTrainer, BandStackedDataset
    nets = [_build_net(q, G, coupling) for q in range(len(BANDS))]
    data = [_build_data(q, G, R) for q in range(len(BANDS))]
    filt = torch.tensor(_band_filters(), device=DEV).to(torch.complex64)
    bank = BandBank(nets)
    tr = BandBankTrainer(bank, _tc(True, **tc), subband_filter_freq_resp=filt, stft_win=WIN, band_names=[int(f) for f in BANDS])
    sds = BandStackedDataset(data)
    start, length = tr._decay_window(NFFT // 2 + 1)
    sds.precompute_decay_targets(WIN, *tr._target_window(NFFT // 2 + 1))
    return nets, data, filt, bank, tr, sds, (start, length)


@pytest.mark.parametrize("G", [3, 4])
def test_coupled_bank_step_equals_band_steps_and_oracle(G):
    """One coupled bank step (normalize, _step_losses, backward, Adam on a fixed Philox mask) == every band's own
    VarReceiverPosTrainer step to rounding, and == the CPU oracle of the reference step with learnable angles."""
    from diffgfdn_amd.trainer import VarReceiverPosTrainer
    from oracle import gfdn_oracle as orc
    from oracle.cpu_trainer import OracleGridTrainer
    nets, data, filt, bank, tr, sds, (start, length) = _bank_setup(G)
    nb = len(BANDS)
    assert bank.coupled and tuple(bank.feedback_loop_alpha.shape) == (nb, G * (G - 1) // 2)
    mw_np, _ = philox_mask(99, 0, length, 1.0 / 4)
    mw = torch.tensor(mw_np, device=DEV)
    sd0 = [{k: v.detach().cpu().clone() for k, v in net.state_dict().items()} for net in nets]
    assert all("feedback_loop.alpha" in sd for sd in sd0)

    batch = sds.collate(sds.global_rows(SELS))
    tr.normalize(batch)
    tr.optimizer.zero_grad(set_to_none=True)
    losses = tr._step_losses(batch, mask_prenorm=mw, defer_total=True)
    heads = losses.pop("_heads")
    torch.autograd.backward(heads, [torch.ones(nb, device=DEV)] * 2)
    tr.optimizer.step()
    got = {k: v.detach().cpu().numpy() for k, v in losses.items()}
    assert got["edr_loss"].shape == (nb,)
    for q in range(nb):                       # the angles took part in the step: every one of them moved
        a1 = nets[q].state_dict()["feedback_loop.alpha"].detach().cpu()
        assert bool((a1 != sd0[q]["feedback_loop.alpha"]).all()), q
        assert torch.equal(a1, bank.feedback_loop_alpha.detach().cpu()[q])

    worst_loss = worst_state = 0.0
    for q in range(nb):
        ref_net = _build_net(q, G)
        ref_net.load_state_dict(sd0[q], strict=True)
        rtr = VarReceiverPosTrainer(ref_net, _tc(True), subband_filter_freq_resp=filt[q], stft_win=WIN, capturable=True)
        ds = data[q]
        ds.precompute_decay_targets(WIN, start, length)
        b = ds.collate(SELS[q], lean=True)
        rtr.normalize(b)
        rtr.optimizer.zero_grad(set_to_none=True)
        rl = rtr._step_losses(b, mask_prenorm=mw)
        rl.pop("_total").backward()
        rtr.optimizer.step()
        for k, v in rl.items():
            e = abs(float(v) - got[k][q]) / abs(float(v))
            worst_loss = max(worst_loss, e)
            within(e, BAND_LOSS_BOUND, ("coupled bank vs band", G, q, k))
        for k, v in ref_net.state_dict().items():
            e = rel_err(nets[q].state_dict()[k].detach().cpu(), v.detach().cpu())
            worst_state = max(worst_state, e)
            within(e, BAND_STATE_BOUND, ("coupled bank vs band", G, q, k))
    print(f"[coupled bank] G = {G}: bank vs band trainers: losses {worst_loss:.3e}, post-Adam state {worst_state:.3e}")

    keep = torch.argwhere(torch.tensor(mw_np) > 0)
    cfg = tr.config
    for q in range(nb):
        dq = data[q]
        sd = sd0[q]
        lin, norm = [], []
        for i in range(64):
            k = f"output_scalars.mlp.model.{i}.weight"
            if k in sd:
                (lin if sd[k].ndim == 2 else norm).append((sd[k].clone(), sd[f"output_scalars.mlp.model.{i}.bias"].clone()))
        p = orc.GridModelParams(FS, _delays(q, G), G, sd["input_gains"].clone(), sd["output_gains"].clone(),
                                sd["feedback_loop.M"].clone(), sd["feedback_loop.alpha"].clone(),
                                np.linspace(0.2, 0.5, G)[None, :], lin, norm, 4)
        otr = OracleGridTrainer(p, lr=1e-3, io_lr=1e-2, edr_weight=1.0, edc_weight=10.0, spectral_weight=1.0,
                                sparsity_weight=2.0, use_asym=True, win=WIN, hop=WIN // 2,
                                subband_filter=filt[q].cpu().to(torch.complex128), learn_alpha=True,
                                coupling_angle_lr=cfg.coupling_angle_lr)
        idx = torch.tensor(SELS[q])
        ob = {"z_values": dq.z_values.cpu(),
              "norm_listener_position": dq.norm_listener_position[idx].cpu(),
              "listener_position": dq.listener_positions[idx].cpu(),
              "target_early_response": dq.early_response_c128(idx).cpu(),
              "target_rir_response": dq.rir_mag_response[idx].cpu().to(torch.complex128)}
        otr.normalize(ob)
        _, oparts = otr.train_step(ob, keep)
        for k, v in oparts.items():
            within(abs(got[k][q] - v), 1e-4 * abs(v) + 1e-7, ("coupled bank vs oracle", G, q, k))
        for name in ("input_gains", "output_gains"):
            within(rel_err(getattr(nets[q], name).detach().cpu(), getattr(p, name).detach()), 1e-4,
                   ("coupled bank vs oracle", G, q, name))
        within(rel_err(nets[q].feedback_loop.alpha.detach().cpu(), p.alpha.detach()), 1e-4,
               ("coupled bank vs oracle", G, q, "feedback_loop.alpha"))


def test_coupled_bank_has_no_explicit_step_and_zero_coupling_keeps_it():
    from diffgfdn_amd.bankstep import FusedBankStep
    from diffgfdn_amd.bandbank import BandBank, BandBankTrainer
    filt = torch.tensor(_band_filters(), device=DEV).to(torch.complex64)
    bank = BandBank([_build_net(q, 3) for q in range(len(BANDS))])
    with pytest.warns(RuntimeWarning, match="inter-group coupling"):
        tr = BandBankTrainer(bank, _tc(True), subband_filter_freq_resp=filt, stft_win=WIN, band_names=BANDS)
    assert tr._fused is None
    assert [g["lr"] for g in tr.optimizer.param_groups] == [1e-2, 1e-2, 1e-3, tr.config.coupling_angle_lr, 1e-2]
    assert tr.optimizer.param_groups[3]["params"][0] is bank.feedback_loop_alpha
    # output_scalars_w still closes the flat buffers
    assert tr.optimizer.flat_range(bank.output_scalars_w)[1] == tr.optimizer.flat_param.numel()
    # zero coupling after the change: the explicit step, no angle leaf, the four groups it always had
    zbank = BandBank([_build_net(q, 3, "zero") for q in range(len(BANDS))])
    ztr = BandBankTrainer(zbank, _tc(True), subband_filter_freq_resp=filt, stft_win=WIN, band_names=BANDS)
    assert isinstance(ztr._fused, FusedBankStep)
    assert not zbank.coupled and not hasattr(zbank, "feedback_loop_alpha")
    assert [n for n, _ in zbank.named_parameters()] == ["input_gains", "output_gains", "feedback_loop_M", "output_scalars_w"]
    assert len(ztr.optimizer.param_groups) == 4
    for g, p in zip(ztr.optimizer.param_groups, (zbank.output_gains, zbank.input_gains, zbank.feedback_loop_M,
                                                 zbank.output_scalars_w)):
        assert g["params"][0] is p


def test_bank_refuses_mixed_and_filter_coupled_bands():
    from diffgfdn_amd.bandbank import BandBank
    with pytest.raises(ValueError, match="mix"):
        BandBank([_build_net(0, 3), _build_net(1, 3, "zero")])
    with pytest.raises(ValueError, match="mix"):
        BandBank([_build_net(0, 3, "zero"), _build_net(1, 3)])
    with pytest.raises(NotImplementedError):
        BandBank([_build_net(0, 3), _build_net(1, 3, "filter")])
    with pytest.raises(NotImplementedError):
        BandBank([_build_net(0, 3, "filter")])


@pytest.mark.parametrize("G", [3, 4])
def test_graphed_coupled_bank_step_equals_eager_step(G):
    nets, data, filt, bank, tr, sds, (start, length) = _bank_setup(G)
    nb = len(BANDS)
    sel_steps = [[[0, 3, 5, 7], [1, 2, 8, 11], [4, 6, 9, 10]],
                 [[1, 2, 4, 6], [0, 5, 7, 9], [3, 8, 10, 11]],
                 [[8, 9, 10, 11], [3, 4, 6, 10], [0, 1, 2, 5]]]
    alpha0 = bank.feedback_loop_alpha.detach().cpu().clone()
    step = tr.graphed(sds, 4, mask_seed=777).capture(sds.global_rows(sel_steps[0]))
    assert torch.equal(bank.feedback_loop_alpha.detach().cpu(), alpha0)        # (the warm-up leaves no trace)
    got, got_grad = [], []
    for s in sel_steps:
        got.append(step(sds.global_rows(s))["_total"].detach().cpu().numpy().copy())
        got_grad.append(tr.optimizer.flat_grad.detach().cpu().numpy().copy())
    assert int(step.mask_state.item()) == len(sel_steps)

    nets2, data2, filt2, bank2, tr2, sds2, _ = _bank_setup(G)
    assert tr2._fused is None
    want = []
    for i, s in enumerate(sel_steps):
        b = sds2.collate(sds2.global_rows(s))
        mw = torch.tensor(philox_mask(777, i, length, 1.0 / 4)[0], device=DEV)
        tr2.optimizer.zero_grad(set_to_none=True)
        losses = tr2._step_losses(b, mask_prenorm=mw, defer_total=True, normalize_first=True)       # as the graph does
        heads = losses.pop("_heads")
        torch.autograd.backward(heads, [torch.ones(nb, device=DEV)] * 2)
        tr2.optimizer.pack_grads()
        total = heads[0].detach() + heads[1].detach()
        if i == 0:
            # same state, same inputs: the replayed gradients are the eager ones to the last bit
            assert np.array_equal(tr2.optimizer.flat_grad.cpu().numpy(), got_grad[0])
        tr2.optimizer.step()
        want.append(total.cpu().numpy())
    for a, b in zip(got, want):
        assert np.allclose(a, b, rtol=1e-5, atol=0), (got, want)
    for q in range(nb):
        for k, v in nets[q].state_dict().items():
            within(rel_err(v.detach().cpu(), nets2[q].state_dict()[k].detach().cpu()), 1e-6, ("coupled graph", G, q, k))
    # the angles of the replayed bank moved with the steps
    assert bool((bank.feedback_loop_alpha.detach().cpu() != alpha0).all())


def test_coupled_bank_training_loop_and_checkpoints(tmp_path):
    nets, data, filt, bank, tr, sds, _ = _bank_setup(3, R=14, max_epochs=2)
    tr.train_dir = str(tmp_path)
    g = torch.Generator().manual_seed(0)
    splits = [torch.randperm(14, generator=g).tolist() for _ in BANDS]
    train = [s[:10] for s in splits]           # 2 full batches + a ragged tail of 2 per band
    valid = [s[10:] for s in splits]
    tr.train(sds, train, valid, batch_size=4, log=False)
    assert len(tr.train_loss[0]) == 2 and all(np.isfinite(tr.train_loss[q]).all() for q in range(len(BANDS)))
    for q, f in enumerate(BANDS):
        ckpt = tmp_path / f"band_{int(f)}" / "checkpoints"
        assert (ckpt / "model_e-1.pt").exists() and (ckpt / "model_e0.pt").exists()
        sd = torch.load(ckpt / "model_e1.pt")
        fresh = _build_net(q, 3)
        fresh.load_state_dict(sd, strict=True)                          # reference-shaped keys, the angles among them
        assert torch.equal(fresh.feedback_loop.alpha.detach().cpu(), bank.feedback_loop_alpha.detach().cpu()[q])
        for k, v in nets[q].state_dict().items():
            assert torch.equal(v.cpu(), sd[k].cpu()), (q, k)
        pd = nets[q].feedback_loop.get_param_dict()
        Phi = np.asarray(pd["coupling_matrix"], dtype=np.float64)
        assert Phi.shape == (3, 3) and np.array_equal(pd["coupling_coefficient"], sd["feedback_loop.alpha"].cpu().numpy())
        within(np.abs(Phi @ Phi.T - np.eye(3)).max(), 1e-5, ("coupled Phi orthogonal", q))
        # the matrices the bank's last forward kept are those of a coupling, too
        kept = bank.coupling_matrices[q].detach().cpu().numpy().astype(np.float64)
        within(np.abs(kept @ kept.T - np.eye(3)).max(), 1e-5, ("coupled Phi kept", q))
