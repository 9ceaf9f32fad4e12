"""GPU (-m gpu): the training step of the second stage -- train_pipeline.pipeline_forward / loss_and_sums / train_step behind a frozen first stage, and
`python -m garmentnets_amd.train_pipeline` end to end.

The error rule is grad_reference._check: ours against torch-fp64 on the CPU <= 4 x (torch-fp32 on the CPU against the same fp64) + 1 fp32 ulp of the
largest gradient; every ratio is printed, no tensor is left out.  The restatement is tests/pipeline_train_reference.py's (held to a direct composition of
torch.nn layers in tests/test_train_pipeline_host.py).  It is handed the rows and cells of ops.grid_features (data) and the ReLU masks of the HIP forward;
the max winners (scatter max, max-pool) are each side's own.

The small models (test_train_pipeline_host.small_hparams): first stage feature_dim 16 / nocs_bins 8 on garments of 200 and 137 points (the smallest for
which the third sampling level keeps >= 2 points; synthetic.plant_nocs_path makes its NOCS prediction follow the points' random colours, so a garment
spreads over a hundred and more of the 512 cells and some cells hold several points), aggregator [25, 25, 16] into 8^3, a two-level UNet 16 -> 16 with
f_maps (16, 48), decoders [16, 32, 32, 1 | 3 | 1], 96 / 80 / 64 queries per garment (three different counts: a mixed-up head shows), a few of them exactly on 0 and 1.
  (A) max, l2, two heads;  (B) mean, smooth_l1, BCE on the volume, the mc head at 0.5, task space, a third garment of 61 points.

BatchNorm buffers: each of the three steps is held to nn.BatchNorm1d in fp64 started from the fp32 buffers THAT step starts from (2 ulp, the BatchNorm
suite's tolerance for one update).  The buffers are fp32 and round once per update, torch's too; a reference that keeps its fp64 state across the three
updates is up to 4 ulp away from either (measured), which is its own drift and not what this asserts.

Measured (MI355X, default arithmetic): the loss against fp64 7.6e-08 / 2.7e-08 (A: train / eval) and 7.1e-08 / 6.4e-08 (B) relative; ours / torch-fp32
over all trainable tensors (A: 52, 337 points in 270 cells; B: 64, 398 points in 246 cells): A 0.13 - 2.41 (train), 0.29 - 1.34 (eval); B 0.18 - 2.28,
0.05 - 2.31; the aggregator's first BatchNorm 0 ulp in each of the three steps; twenty steps take the loss from 0.4762 to 0.0754.  The command-line test
adds `--volume_size` (the test store holds one volume size) to the arguments of the issue.
"""
import copy
import csv
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import ops, synthetic, train_pipeline as TP  # noqa: E402
from garmentnets_amd.batch import Batch  # noqa: E402
from garmentnets_amd.networks.conv_implicit_wnf import ConvImplicitWNFPipeline  # noqa: E402
from garmentnets_amd.networks.pointnet2_nocs import PointNet2NOCS  # noqa: E402
from garmentnets_amd.optim import FusedAdam  # noqa: E402
from grad_reference import _check, _gen  # noqa: E402
import pipeline_train_reference as PR  # noqa: E402
from test_train_pipeline_host import small_model, targets  # noqa: E402

DEV = "cuda:0"
CONFIGS = {"A": (dict(reduce_method="max"), [200, 137]),
           "B": (dict(reduce_method="mean", mc=0.5, loss_type="smooth_l1", volume_classification=True, volume_task_space=True), [200, 137, 61])}
AABB = torch.tensor([[[-0.4, -0.4, -0.9], [0.4, 0.4, 0.05]]])
FIRST = "pointnet2_nocs."


def _bits(a, b):
    a, b = a.float(), b.float()
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _setup(config, seed=1, batch_seed=41):
    """-> (the CPU model, the host batch).  In task space the cloud lies inside the store's bounding box, so the normalised positions fill the unit cube"""
    kw, sizes = CONFIGS[config]
    g = _gen(batch_seed)
    n, nb = sum(sizes), len(sizes)
    pos = torch.rand(n, 3, generator=g)
    if kw.get("volume_task_space"):
        pos = pos * torch.tensor([0.7, 0.7, 0.9]) + torch.tensor([-0.35, -0.35, -0.88])
    t = targets(nb, batch_seed + 1, binary_volume=kw.get("volume_classification", False))
    batch = Batch(sizes=sizes, x=torch.rand(n, 3, generator=g), pos=pos, batch=torch.arange(nb).repeat_interleave(torch.tensor(sizes)),
                  cloth_sim_aabb=AABB.repeat(nb, 1, 1), **vars(t))
    return small_model(seed, planted_nocs=True, **kw), batch


def _first_stage_relus(model, batch):
    """how many bare-ReLU gn_linear calls the frozen first stage makes (its lin1): the recorder's entries before the second stage's"""
    with PR.record_second_stage() as rec:
        p2 = TP.first_stage(model, batch)
    return len(rec["r"]), p2


def _head_outputs(result):
    out = {k: result[k]["out_features"] for k in ("volume_decoder_result", "surface_decoder_result", "mc_surface_decoder_result") if k in result}
    out["pred_volume_value"] = result["volume_decoder_result"]["pred_volume_value"]
    out["out_feature_volume"] = result["unet3d_result"]["out_feature_volume"]
    out["per_point_logits"] = result["pointnet2_result"]["per_point_logits"]
    return out


def _same_results(a, b):
    a, b = _head_outputs(a), _head_outputs(b)
    return set(a) == set(b) and all(_bits(a[k], b[k]) for k in a)


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return set(sa) == set(sb) and all(_bits(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------------------------------------ 1. the whole model's gradient
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("config", ["A", "B"])
def test_whole_model_gradient(config, mode):
    cpu_model, batch_cpu = _setup(config)
    model = copy.deepcopy(cpu_model).to(DEV).requires_grad_(True)
    model.train(mode == "train")
    batch = batch_cpu.to(DEV)
    buffers = {k: v.detach().cpu().clone() for k, v in model.named_buffers()}
    skip, p2 = _first_stage_relus(model, batch)
    nd, agg = p2["nocs_data"], model.volume_agg
    rows, flat = ops.grid_features(nd.x, nd.pos.contiguous(), nd.sim_points.float().contiguous(), nd.pred_confidence.contiguous(), nd.batch,
                                   agg.lower_corner, agg.upper_corner, agg.grid_shape, True, True)
    rows, flat = rows.cpu().contiguous(), flat.cpu()
    occupied = len(torch.unique(flat))
    print(f"[train-pipeline] whole model ({config}, {mode}): {flat.numel()} points in {occupied} cells")
    assert rows.shape[1] == 25 and 50 * len(batch_cpu.sizes) < occupied < flat.numel()      # the points spread over the cells; some cells are shared
    with PR.record_second_stage() as rec:
        result = TP.pipeline_forward(model, batch)
        loss, _ = TP.loss_and_sums(model, batch, result)
    loss.backward()
    heads = 3 if config == "B" else 2
    assert len(rec["r"]) == skip + 2 + 3 * heads and len(rec["conv"]) == 6
    assert set(result) == {"pointnet2_result", "unet3d_result", "volume_decoder_result", "surface_decoder_result"} | \
        ({"mc_surface_decoder_result"} if config == "B" else set())
    assert tuple(result["volume_decoder_result"]["pred_volume_value"].shape) == (len(batch_cpu.sizes), 96)
    masks = ([(r > 0).cpu() for r in rec["r"][skip:]], rec["conv"])

    def restated(dtype):
        P = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in model.named_parameters() if not k.startswith(FIRST)}
        ls = PR.Restated(cpu_model, P, buffers, dtype, mode == "train", masks).loss(rows, flat, batch_cpu)
        return float(ls.detach()), dict(zip(P, torch.autograd.grad(ls, list(P.values()))))
    l64, g64 = restated(torch.float64)
    l32, g32 = restated(torch.float32)
    print(f"[train-pipeline] whole model ({config}, {mode}): loss fp64 {l64:.9f}  torch-fp32 {l32:.9f}  hip {loss.item():.9f}  "
          f"relative {abs(loss.item() - l64) / abs(l64):.2e}")
    assert abs(loss.item() - l64) <= 1e-5 * abs(l64)
    failed, ratios = [], []
    for name, p in model.named_parameters():
        if name.startswith(FIRST):
            assert p.grad is None, name
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        try:
            ratios.append(_check(f"whole model ({config}, {mode}) {name}", g64[name], g32[name], p.grad))
        except AssertionError as e:
            failed.append(str(e.args[0])[:200])
    assert len(ratios) + len(failed) == len(g64)                                          # every trainable tensor was held to the rule
    if ratios:
        print(f"[train-pipeline] whole model ({config}, {mode}): {len(g64)} tensors, ours / torch-fp32 {min(ratios):.2f} - {max(ratios):.2f}")
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ 2. the frozen first stage
def test_first_stage_stays_frozen_and_batchnorm_tracks():
    cpu_model, batch_cpu = _setup("A")
    model = copy.deepcopy(cpu_model).to(DEV).requires_grad_(True).train()
    batch = batch_cpu.to(DEV)
    before = {k: v.detach().clone() for k, v in model.pointnet2_nocs.state_dict().items()}
    bns = [m for name, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm1d) and not name.startswith(FIRST)]
    tracked = [int(bn.num_batches_tracked) for bn in bns]
    bn0 = model.volume_agg.local_nn[0][2]
    skip, _ = _first_stage_relus(model, batch)
    model.train()
    opt = model.configure_optimizers()
    worst = {"running_mean": 0.0, "running_var": 0.0}
    for step in range(3):
        # nn.BatchNorm1d in fp64, started from the fp32 buffers this step starts from (the buffers are fp32 and round once per update, torch's too)
        ref = torch.nn.BatchNorm1d(bn0.num_features, eps=bn0.eps, momentum=bn0.momentum).double()
        with torch.no_grad():
            ref.running_mean.copy_(bn0.running_mean)
            ref.running_var.copy_(bn0.running_var)
        with PR.record_second_stage() as rec:
            TP.train_step(model, opt, batch)
        with torch.no_grad():
            ref(rec["r"][skip].cpu().double())                                            # the rows the aggregator's first BatchNorm saw in this step
        for k in worst:
            got, want = getattr(bn0, k).cpu().numpy(), getattr(ref, k).float().numpy()
            ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want))
            worst[k] = max(worst[k], float(ulps.max()))
            assert (ulps <= 2).all(), (step, k, float(ulps.max()))                        # test_gpu_bn_train.py::_check_buffers' tolerance
    print(f"[train-pipeline] aggregator block 0 over three steps: largest difference running_mean {worst['running_mean']:.1f} ulp, "
          f"running_var {worst['running_var']:.1f} ulp")
    after = model.pointnet2_nocs.state_dict()
    assert set(after) == set(before) and all(_bits(after[k], before[k]) for k in before)
    assert all(p.grad is None for p in model.pointnet2_nocs.parameters()) and not model.pointnet2_nocs.training
    assert len(bns) == 2 + 3 * 2 and [int(bn.num_batches_tracked) for bn in bns] == [t + 3 for t in tracked]
    # a first-stage parameter holds no optimiser state and its step never advanced
    p1, p2 = next(model.pointnet2_nocs.parameters()), next(model.volume_agg.parameters())
    assert len(opt.state[p1]) == 0 and float(opt.state[p2]["step"]) == 3.0


# ------------------------------------------------------------------------------------------------ 3. one step, end to end
def test_train_step_end_to_end():
    cpu_model, batch_cpu = _setup("B")
    model = copy.deepcopy(cpu_model).to(DEV).requires_grad_(True).train()
    twin = copy.deepcopy(model)
    batch = batch_cpu.to(DEV)
    with torch.no_grad():
        warm = _head_outputs(model.eval()(batch))                                         # the inference packs exist before the step: they must not survive it
        warm = {k: v.clone() for k, v in warm.items()}
    model.train()
    metrics = TP.train_step(model, model.configure_optimizers(), batch)
    assert set(metrics) == set(TP.metric_keys(model)) == {"loss", "volume_loss", "surface_loss", "mc_surface_loss"}
    assert all(math.isfinite(v) for v in metrics.values())
    opt2 = FusedAdam(twin.parameters(), lr=twin.learning_rate)
    opt2.zero_grad(set_to_none=True)
    loss = twin.training_step(batch)
    loss.backward()
    opt2.step()
    assert np.float32(metrics["loss"]) == np.float32(loss.item())
    assert _same_state(model, twin)
    # the very next inference forward reads the new weights: forward's bits are those of a model freshly loaded with the trained state
    kw, _ = CONFIGS["B"]
    fresh = small_model(7, **kw).to(DEV)                                                  # (other weights: every tensor comes from the state dict)
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        out = model.eval()(batch)
        composed = TP.pipeline_forward(model, batch)
        ref = fresh.eval()(batch)
    assert _same_results(out, composed) and _same_results(out, ref)
    now = _head_outputs(out)
    assert all(not torch.equal(now[k], warm[k]) for k in warm if k != "per_point_logits")
    assert _bits(now["per_point_logits"], warm["per_point_logits"])                       # the frozen first stage's output is the pre-step one


# ------------------------------------------------------------------------------------------------ 4. eval mode without a gradient
@pytest.mark.parametrize("config", ["A", "B"])
def test_eval_without_gradient_is_forward(config):
    cpu_model, batch_cpu = _setup(config)
    model = copy.deepcopy(cpu_model).to(DEV).requires_grad_(True).eval()
    batch = batch_cpu.to(DEV)
    with torch.no_grad():
        a, b = TP.pipeline_forward(model, batch), model(batch)
        assert _same_results(a, b)
        assert model.training_metrics(batch) == model.validation_metrics(batch)
    model.requires_grad_(False)                                                            # nothing wants a gradient: the same, with autograd switched on
    c = TP.pipeline_forward(model, batch)
    assert _same_results(c, b) and not c["surface_decoder_result"]["out_features"].requires_grad


# ------------------------------------------------------------------------------------------------ 5. twenty steps
def test_twenty_steps_reduce_the_loss_and_repeat_bit_for_bit():
    cpu_model, batch_cpu = _setup("A", seed=9, batch_seed=43)
    batch = batch_cpu.to(DEV)
    start = cpu_model.to(DEV).requires_grad_(True).eval()                                  # eval-mode BatchNorm: a fixed objective

    def run():
        model = copy.deepcopy(start)
        opt = FusedAdam(model, lr=1e-3)
        losses = [TP.train_step(model, opt, batch)["loss"] for _ in range(20)]
        return losses, model
    la, ma = run()
    lb, mb = run()
    print(f"[train-pipeline] twenty steps: loss {la[0]:.6f} -> {la[-1]:.6f}")
    assert la[-1] < la[0]
    assert la == lb and _same_state(ma, mb)


# ------------------------------------------------------------------------------------------------ 6. the command line
def test_train_pipeline_main_end_to_end(tmp_path):
    from test_validate_host import VOLUME_SIZE, write_validation_store
    store, out_dir = tmp_path / "ds.zarr", tmp_path / "out"
    write_validation_store(str(store), 20)
    common = ["--zarr_in", str(store), "--volume_size", str(VOLUME_SIZE), "--epochs", "1", "--batch_size", "2", "--num_pc_sample", "400",
              "--num_volume_sample", "96", "--num_surface_sample", "80", "--grid", "8"]
    res = TP.main(common + ["--output_dir", str(out_dir), "--num_batches", "2"])
    rows = list(csv.DictReader(open(out_dir / "train_metrics.csv")))
    cols = {"epoch", "batch_idx", "garments", "data_seconds", "seconds", "train_loss", "train_volume_loss", "train_surface_loss"}
    assert len(rows) == 2 and set(rows[0]) == cols and all(math.isfinite(float(v)) for r in rows for v in r.values())
    assert all(float(r["data_seconds"]) > 0 for r in rows)
    assert (out_dir / "val_epochs.json").exists() and len(res["val_epochs"]) == 1 and math.isfinite(res["val_epochs"][0]["val_loss"])
    ck = out_dir / "checkpoints" / "last.ckpt"
    loaded = ConvImplicitWNFPipeline.load_from_checkpoint(str(ck))
    trained = res["model"].state_dict()
    assert set(loaded.state_dict()) == set(trained)
    assert all(torch.equal(v.cpu(), trained[k].cpu()) for k, v in loaded.state_dict().items())
    saved = torch.load(str(ck), map_location="cpu", weights_only=False)
    assert saved["epoch"] == 0 and set(saved) >= {"state_dict", "hyper_parameters", "optimizer_states", "epoch"}
    opt = FusedAdam(loaded.parameters())
    opt.load_state_dict(saved["optimizer_states"][0])
    second, first = next(loaded.volume_agg.parameters()), next(loaded.pointnet2_nocs.parameters())
    assert float(opt.state[second]["step"]) == 2.0 and opt.state[second]["exp_avg"].shape == second.shape
    assert len(opt.state[first]) == 0
    # the first stage from a checkpoint of its own: the second stage keeps its constructors' initialisation under --seed
    hp = synthetic.default_hparams()
    p2 = PointNet2NOCS(**hp["pointnet2_params"])
    p2.load_state_dict({k[len(FIRST):]: v for k, v in synthetic.synthetic_state_dict(hp, 4).items() if k.startswith(FIRST)})
    p2.save_checkpoint(str(tmp_path / "p2.ckpt"))
    res2 = TP.main(common + ["--output_dir", str(tmp_path / "out2"), "--num_batches", "1", "--pointnet2_checkpoint", str(tmp_path / "p2.ckpt"), "--seed", "3"])
    got, want = res2["model"].pointnet2_nocs.state_dict(), p2.state_dict()
    assert set(got) == set(want) and all(_bits(got[k].cpu(), want[k]) for k in want)
    assert res2["model"].hparams["pointnet2_params"] == p2.hparams
    torch.manual_seed(3)
    init = ConvImplicitWNFPipeline(**synthetic.default_hparams(grid=8))
    w0 = init.unet_3d.abstract_3d_unet.final_conv.weight
    w1 = res2["model"].unet_3d.abstract_3d_unet.final_conv.weight.detach().cpu()
    assert w0.shape == w1.shape and float((w0 - w1).abs().max()) <= 2e-4                  # one Adam step of lr 1e-4 away from the seeded initialisation
    assert math.isfinite(res2["train_rows"][0]["train_loss"])
