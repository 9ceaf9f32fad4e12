"""Host side of the second stage's training step (no GPU): the command line of garmentnets_amd.train_pipeline, the one segment list validation and the
step share, configure_optimizers' group, and tests/pipeline_train_reference.py itself -- its fp64 loss against a direct composition of torch.nn layers on
a tiny case, which shows that the restatement the GPU suite compares against is the model."""
import itertools
import types

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from garmentnets_amd import synthetic
from garmentnets_amd import train_pipeline as TP
from garmentnets_amd.networks.conv_implicit_wnf import ConvImplicitWNFPipeline
from grad_reference import _gen
import pipeline_train_reference as PR


def small_hparams(reduce_method="max", mc=0.0, **kw):
    """the small model of the GPU suite: every width the smallest at which its branch is live"""
    hp = dict(pointnet2_params=dict(feature_dim=16, batch_norm=True, dropout=False, sa1_ratio=0.5, sa1_r=0.25, sa2_ratio=0.25, sa2_r=0.5, fp3_k=1,
                                    fp2_k=3, fp1_k=3, nocs_bins=8),
              volume_agg_params=dict(nn_channels=[25, 25, 16], batch_norm=True, lower_corner=[0, 0, 0], upper_corner=[1, 1, 1], grid_shape=[8, 8, 8],
                                     reduce_method=reduce_method, include_point_feature=True, include_confidence_feature=True),
              unet3d_params=dict(in_channels=16, out_channels=16, f_maps=(16, 48), layer_order="gcr", num_groups=8, num_levels=2),
              volume_decoder_params=dict(nn_channels=[16, 32, 32, 1], batch_norm=True),
              surface_decoder_params=dict(nn_channels=[16, 32, 32, 3], batch_norm=True),
              mc_surface_decoder_params=dict(nn_channels=[16, 32, 32, 1], batch_norm=True), mc_surface_loss_weight=mc, learning_rate=1e-3)
    hp.update(kw)
    return hp


def small_model(seed=0, planted_nocs=False, **kw):
    """planted_nocs: synthetic.plant_nocs_path -- the first stage predicts the NOCS bin nearest to each point's colour, so a cloud with random colours
    spreads over the cells of the grid (seeded random weights alone put a whole garment into two or three cells)"""
    hp = small_hparams(**kw)
    model = ConvImplicitWNFPipeline(**hp)
    model.load_state_dict(synthetic.synthetic_state_dict(hp, seed, planted_nocs=planted_nocs))
    return model


def targets(nb, seed, counts=(96, 80, 64), binary_volume=False):
    """query points (a few exactly on 0 and 1) and seeded random targets, in the shapes io.dataset collates; mc targets in {0, 1}"""
    g = _gen(seed)
    mv, ms, mm = counts
    edge = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 0.5]])
    q = [torch.rand(nb, m, 3, generator=g) for m in counts]
    for t in q:
        t[:, :3] = edge
    gv = torch.rand(nb, mv, generator=g)
    return types.SimpleNamespace(volume_query_points=q[0], surf_query_points=q[1], mc_surf_query_points=q[2],
                                 gt_volume_value=(gv > 0.5).float() if binary_volume else gv,
                                 gt_sim_points=0.3 * torch.randn(nb, ms, 3, generator=g),
                                 is_query_point_on_surf=(torch.rand(nb, mm, 1, generator=g) > 0.5).float())


# ------------------------------------------------------------------------------------------------ the command line
def test_parser_defaults_are_the_pipeline_config():
    a = TP.parse_args(["--zarr_in", "x.zarr"])
    assert (a.model, a.batch_size, a.subset, a.epochs, a.learning_rate, a.seed) == ("pipeline", 24, "train", 1, None, 0)
    assert (a.checkpoint_path, a.pointnet2_checkpoint) == (None, None)
    assert (a.num_pc_sample, a.num_volume_sample, a.num_surface_sample, a.num_mc_surface_sample, a.grid, a.reduce_method) == (6000, 6000, 6000, 0, 32, "max")


def test_parser_takes_both_checkpoints_and_refuses_the_first_stage():
    a = TP.parse_args(["--zarr_in", "x.zarr", "--pointnet2_checkpoint", "p2.ckpt", "--checkpoint_path", "pipe.ckpt", "--epochs", "3", "--learning_rate",
                       "1e-3", "--seed", "7"])
    assert (a.pointnet2_checkpoint, a.checkpoint_path, a.epochs, a.learning_rate, a.seed) == ("p2.ckpt", "pipe.ckpt", 3, 1e-3, 7)
    with pytest.raises(SystemExit) as e:
        TP.parse_args(["--zarr_in", "x.zarr", "--model", "pointnet2"])
    assert "garmentnets_amd.train" in str(e.value)


# ------------------------------------------------------------------------------------------------ the segments
@pytest.mark.parametrize("loss_type,classification,mc", list(itertools.product(("l2", "smooth_l1"), (False, True), (0, 0.5))))
def test_loss_segments_are_losses_froms(loss_type, classification, mc):
    """the helper hands losses_from what losses_from formed itself before the refactoring, written out here: tensors, kinds, names, weights, order"""
    model = ConvImplicitWNFPipeline(**small_hparams(mc=mc), loss_type=loss_type, volume_classification=classification, volume_loss_weight=0.7,
                                    surface_loss_weight=1.3)
    t = targets(2, 3)
    pv, ps, pm = torch.zeros(2, 96), torch.zeros(2, 80, 3), torch.zeros(2, 64, 1)
    result = {"volume_decoder_result": {"pred_volume_value": pv}, "surface_decoder_result": {"out_features": ps}}
    if mc:
        result["mc_surface_decoder_result"] = {"out_features": pm}
    want = [(pv, t.gt_volume_value, "bce_logits" if classification else loss_type, "volume_loss", 0.7), (ps, t.gt_sim_points, loss_type, "surface_loss", 1.3)]
    if mc:
        want.append((pm, t.is_query_point_on_surf, "bce_logits", "mc_surface_loss", 0.5))
    segs, names, weights = model.loss_segments(result, t)
    assert len(segs) == len(want) and list(names) == [w[3] for w in want] and list(weights) == [w[4] for w in want]
    for seg, w in zip(segs, want):
        assert len(seg) == 3 and seg[0] is w[0] and seg[1] is w[1] and seg[2] == w[2]
    assert TP.metric_keys(model) == ("loss",) + tuple(names)
    # losses_from's expression on the sums
    sums = [3.0, 5.0, 7.0][:len(want)]
    counts = [w[1].numel() for w in want]
    m = model.metrics_from_sums(sums, names, weights, counts)
    parts = [w[4] * (s / n) for w, s, n in zip(want, sums, counts)]
    assert list(m) == list(names) + ["loss"] and [m[k] for k in names] == parts and m["loss"] == sum(parts)


def test_an_unknown_loss_type_is_refused():
    model = ConvImplicitWNFPipeline(**small_hparams(), loss_type="l1")
    with pytest.raises(ValueError, match="Invalid loss_type"):
        model.loss_segments({}, None)


# ------------------------------------------------------------------------------------------------ the optimiser
def test_configure_optimizers_is_one_group_of_every_parameter():
    model = ConvImplicitWNFPipeline(**small_hparams(mc=0.5, learning_rate=3e-4))
    opt = model.configure_optimizers()
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == 3e-4
    ours, every = opt.param_groups[0]["params"], list(model.parameters())
    assert len(ours) == len(every) and all(a is b for a, b in zip(ours, every))
    assert any(p is ours[0] for p in model.pointnet2_nocs.parameters())                   # the frozen first stage's are in the group, as the reference's


# ------------------------------------------------------------------------------------------------ the restatement is the model
class _Block(nn.Sequential):
    def __init__(self, cin, cout):
        super().__init__(nn.Linear(cin, cout), nn.ReLU(), nn.BatchNorm1d(cout))


def _mlp(channels):
    return nn.Sequential(*[_Block(a, b) for a, b in zip(channels[:-1], channels[1:])])


class _Gcr(nn.Module):
    def __init__(self, cin, cout, groups):
        super().__init__()
        self.groupnorm, self.conv = nn.GroupNorm(groups, cin), nn.Conv3d(cin, cout, 3, padding=1, bias=False)

    def forward(self, x):
        return F.relu(self.conv(self.groupnorm(x)))


class _Direct(nn.Module):
    """the second stage as torch.nn layers, for ONE architecture written out: aggregator [25, 25, 16], scatter, a two-level UNet 16 -> 16 with
    f_maps (16, 48), decoders [16, 32, 32, out]"""

    def __init__(self, reduce, mc):
        super().__init__()
        self.reduce = reduce
        self.agg = _mlp([25, 25, 16])
        self.e0 = nn.Sequential(_Gcr(16, 16, 8), _Gcr(16, 16, 8))
        self.e1 = nn.Sequential(nn.MaxPool3d(2), _Gcr(16, 24, 8), _Gcr(24, 48, 8))
        self.up = nn.Upsample(scale_factor=2, mode="nearest")
        self.d0 = nn.Sequential(_Gcr(64, 16, 8), _Gcr(16, 16, 8))
        self.final = nn.Conv3d(16, 16, 1)
        self.decoders = nn.ModuleList([_mlp([16, 32, 32, o]) for o in ((1, 3, 1) if mc else (1, 3))])

    def load(self, sd):
        def mlp(stack, prefix):
            for i, block in enumerate(stack):
                block[0].load_state_dict({k: sd[f"{prefix}.{i}.0.{k}"] for k in ("weight", "bias")})
                block[2].load_state_dict({k: sd[f"{prefix}.{i}.2.{k}"] for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")})
        mlp(self.agg, "volume_agg.local_nn")
        u = "unet_3d.abstract_3d_unet."
        for layers, name in (((self.e0[0], self.e0[1]), "encoders.0"), ((self.e1[1], self.e1[2]), "encoders.1"), ((self.d0[0], self.d0[1]), "decoders.0")):
            for j, layer in enumerate(layers):
                p = f"{u}{name}.basic_module.SingleConv{j + 1}."
                layer.groupnorm.load_state_dict({k: sd[p + "groupnorm." + k] for k in ("weight", "bias")})
                layer.conv.load_state_dict({"weight": sd[p + "conv.weight"]})
        self.final.load_state_dict({k: sd[u + "final_conv." + k] for k in ("weight", "bias")})
        for dec, name in zip(self.decoders, ("volume_decoder", "surface_decoder", "mc_surface_decoder")):
            mlp(dec, name + ".mlp")
        return self

    def forward(self, rows, flat, nb, queries):
        f = self.agg(rows)
        cells = nb * 512
        idx = flat.long()[:, None].expand_as(f)
        if self.reduce == "mean":
            vol = torch.zeros(cells, 16, dtype=f.dtype).scatter_reduce(0, idx, f, "mean", include_self=False)
        else:
            vol = torch.zeros(cells, 16, dtype=f.dtype).scatter_reduce(0, idx, f, "amax", include_self=False)
        x0 = self.e0(vol.view(nb, 8, 8, 8, 16).permute(0, 4, 1, 2, 3))
        out = self.final(self.d0(torch.cat((x0, self.up(self.e1(x0))), 1)))
        preds = []
        for dec, q in zip(self.decoders, queries):
            s = F.grid_sample(out, (2.0 * q - 1.0).view(nb, -1, 1, 1, 3), mode="bilinear", padding_mode="border", align_corners=True)
            s = s.view(nb, 16, -1).permute(0, 2, 1).reshape(-1, 16)
            preds.append(dec(s).view(nb, q.shape[1], -1))
        return preds


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("config", ["A", "B"])
def test_the_restatement_is_the_model(config, training):
    """(A) max, l2, two heads; (B) mean, smooth_l1, BCE on the volume, the mc head at 0.5: the fp64 loss and one gradient of the restatement against
    torch.nn layers composed directly (its own ReLUs: no masks are handed in without a GPU)"""
    kw = dict(reduce_method="max") if config == "A" else dict(reduce_method="mean", mc=0.5, loss_type="smooth_l1", volume_classification=True)
    model = small_model(seed=1, **kw)
    nb, n = 2, 150
    g = _gen(11)
    rows = torch.randn(nb * n, 25, generator=g, dtype=torch.float64)
    cell = torch.randint(0, 8, (nb * n, 3), generator=g)
    cell[:40] = cell[0]                                                                     # one crowded cell
    flat = ((torch.arange(nb).repeat_interleave(n) * 8 + cell[:, 0]) * 8 + cell[:, 1]) * 8 + cell[:, 2]
    t = targets(nb, 12, binary_volume=config == "B")
    sd = model.state_dict()
    direct = _Direct(kw["reduce_method"], config == "B").load(sd).double().train(training)
    preds = direct(rows, flat, nb, [q.double() for q in (t.volume_query_points, t.surf_query_points, t.mc_surf_query_points)])
    crit = F.mse_loss if config == "A" else F.smooth_l1_loss
    want = (F.binary_cross_entropy_with_logits if config == "B" else crit)(preds[0].squeeze(-1), t.gt_volume_value.double()) + \
        crit(preds[1], t.gt_sim_points.double())
    if config == "B":
        want = want + 0.5 * F.binary_cross_entropy_with_logits(preds[2], t.is_query_point_on_surf.double())
    want.backward()
    P = {k: v.detach().double().requires_grad_(True) for k, v in model.named_parameters()}
    buffers = {k: v.detach().clone() for k, v in model.named_buffers()}
    got = PR.Restated(model, P, buffers, torch.float64, training).loss(rows, flat, t)
    got_v, want_v = float(got.detach()), float(want.detach())
    assert abs(got_v - want_v) <= 1e-12 * abs(want_v), (got_v, want_v)
    for name, ref in (("volume_agg.local_nn.0.0.weight", direct.agg[0][0].weight), ("unet_3d.abstract_3d_unet.encoders.1.basic_module.SingleConv2.conv.weight",
                                                                                 direct.e1[2].conv.weight),
                      ("surface_decoder.mlp.2.2.bias", direct.decoders[1][2][2].bias)):
        gr = torch.autograd.grad(got, P[name], retain_graph=True)[0]
        assert float((gr - ref.grad).abs().max()) <= 1e-10 * float(ref.grad.abs().max()), name


@pytest.mark.parametrize("reduce", ["max", "min", "mean", "sum"])
def test_r_scatter_against_scatter_reduce(reduce):
    g = _gen(5)
    src = torch.randn(60, 4, generator=g, dtype=torch.float64)
    flat = torch.randint(0, 9, (60,), generator=g) * 2                                      # odd cells stay empty
    idx = flat[:, None].expand_as(src)
    want = torch.zeros(20, 4, dtype=torch.float64).scatter_reduce(0, idx, src, {"max": "amax", "min": "amin", "mean": "mean", "sum": "sum"}[reduce],
                                                                  include_self=False)
    got = PR.r_scatter(src, flat, 20, reduce)
    assert float((got - want).abs().max()) <= 1e-14 and not bool(got[1::2].any())
