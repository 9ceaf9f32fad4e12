"""GPU (-m gpu): the validation losses of csrc/losses.hip (ops.nocs_bin_metrics, ops.value_losses) against fp32-per-element and all-fp64
torch restatements, the reference's metric dicts of tests/golden/ref_validate.npz, and `python -m garmentnets_amd.validate` end to end on a
synthetic store for both models."""
import csv
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from garmentnets_amd import ops, synthetic as S, validate as V  # noqa: E402
from garmentnets_amd.components.gridding import VirtualGrid  # noqa: E402
from garmentnets_amd.networks.conv_implicit_wnf import ConvImplicitWNFPipeline  # noqa: E402
from garmentnets_amd.networks.pointnet2_nocs import PointNet2NOCS  # noqa: E402
from oracle import pipeline as P  # noqa: E402
from test_validate_host import GOLDEN, write_validation_store  # noqa: E402

DEV = "cuda:0"
TOL = 1e-4            # the decoder bound of test_gpu_api.py::test_forward_with_explicit_query_sets_against_oracle


def sqrt_rn(x):
    """correctly rounded fp32 square root (fp64 root rounded once: exact for fp32 inputs), as the kernels take it"""
    return torch.sqrt(x.double()).float()


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ------------------------------------------------------------------------------------------------ gn_nocs_bin_metrics
def bin_inputs(n, bins, seed):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(n, bins, 3, generator=g) * 4
    lg[::7] = torch.round(lg[::7])                                      # exact ties: the first maximum wins
    lg[3::11] *= 20                                                      # magnitudes up to ~80
    lg = lg.clamp(-80, 80)
    gt = torch.rand(n, 3, generator=g)
    edges = torch.tensor([0.0, 1.0] + [k / max(bins - 1, 1) for k in range(bins)], dtype=torch.float32)
    pick = torch.randint(0, len(edges), (n, 3), generator=g)
    on_edge = torch.rand(n, 3, generator=g) < 0.3
    gt = torch.where(on_edge, edges[pick], gt)                         # targets on bin edges 0, 1, k/(bins-1)
    return lg.reshape(n, bins * 3).to(DEV), gt.to(DEV)


def mirror(p, axis):
    if axis is None:
        return p
    q = p.clone()
    q[:, axis] = (q[:, axis] - 0.5) * -1 + 0.5                          # fp32, each step rounded (torch does not fuse)
    return q


def bin_restatement(lg, gt, bins, axis):
    """-> ([ce, ce_m, dist, dist_m] with fp32 per-element terms summed in fp64, the same with fp64 terms)"""
    n = lg.shape[0]
    l3 = lg.reshape(n, bins, 3)
    vg = VirtualGrid(grid_shape=(bins,) * 3, batch_size=1, device=lg.device)
    gtm = mirror(gt, axis)
    t, tm = vg.get_points_grid_idxs(gt), vg.get_points_grid_idxs(gtm)
    idx, _, pred = ops.nocs_head(lg, bins)                             # first-maximum arg-max -> coordinate
    assert torch.equal(idx, torch.argmax(l3, dim=1))                   # gn_nocs_head's rule is torch's: the first maximum
    mx = l3.max(dim=1).values
    s = torch.zeros_like(mx)
    for k in range(bins):
        s = s + torch.exp(l3[:, k, :] - mx)
    lse = torch.log(s)
    ce32 = lse - (torch.gather(l3, 1, t[:, None, :]).squeeze(1) - mx)
    cem32 = lse - (torch.gather(l3, 1, tm[:, None, :]).squeeze(1) - mx)

    def norm32(d):
        return sqrt_rn((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])

    f32 = [ce32.double().sum(), cem32.double().sum(), norm32(pred - gt).double().sum(), norm32(pred - gtm).double().sum()]
    l64 = l3.double()
    ce64 = F.cross_entropy(l64, t, reduction="sum")
    cem64 = F.cross_entropy(l64, tm, reduction="sum")
    p64 = vg.idxs_to_points(idx).double()
    f64 = [ce64, cem64, torch.linalg.norm(p64 - gt.double(), dim=1).sum(), torch.linalg.norm(p64 - gtm.double(), dim=1).sum()]
    return [float(v) for v in f32], [float(v) for v in f64], t, tm


@pytest.mark.parametrize("bins", [64, 17, 1])
@pytest.mark.parametrize("n", [1, 255, 6000 * 8])
@pytest.mark.parametrize("axis", [None, 0, 1, 2])
def test_nocs_bin_metrics_against_restatements(bins, n, axis):
    lg, gt = bin_inputs(n, bins, seed=bins * 1000 + n + (axis or 0))
    out = ops.nocs_bin_metrics([(lg, gt)], bins, axis).cpu().numpy()[0]
    f32, f64, t, tm = bin_restatement(lg, gt, bins, axis)
    # binning: bins k/(bins-1) are edges, the target bin is VirtualGrid's (a wrong bin moves CE by whole units)
    assert int(t.min()) >= 0 and int(t.max()) <= bins - 1
    if axis is None:
        np.testing.assert_array_equal(out[[1, 3]], out[[0, 2]])
    for j in range(4):
        if bins == 1 and j >= 2:            # one bin: the coordinate is 0 * (1 / 0) = NaN, as VirtualGrid.idxs_to_points gives
            assert np.isnan(out[j]) and np.isnan(f32[j])
            continue
        assert rel(out[j], f32[j]) <= 1e-9, (j, out[j], f32[j])
        assert rel(out[j], f64[j]) <= 1e-6, (j, out[j], f64[j])


def test_nocs_bin_metrics_several_sets_strided_rows_and_bits():
    """the per-point rows (padded leading dimension, as lin3 writes them) and the global rows in ONE launch; identical calls, identical bits"""
    bins = 64
    lg, gt = bin_inputs(6000 * 8, bins, seed=5)
    buf = torch.zeros(lg.shape[0], bins * 3 + 4, device=DEV)
    buf[:, :bins * 3] = lg
    glg, ggt = bin_inputs(8, bins, seed=6)
    a = ops.nocs_bin_metrics([(buf[:, :bins * 3], gt), (glg, ggt)], bins, 0)
    b = ops.nocs_bin_metrics([(lg, gt), (glg, ggt)], bins, 0)
    c = ops.nocs_bin_metrics([(lg, gt), (glg, ggt)], bins, 0)
    assert torch.equal(a, b) and torch.equal(b, c)
    assert torch.equal(b[1], ops.nocs_bin_metrics([(glg, ggt)], bins, 0)[0])


# ------------------------------------------------------------------------------------------------ gn_value_losses
def value_restatement(p, t, kind, mirror_x):
    if mirror_x:
        t = t.reshape(-1, 3).clone()
        t[:, 0] = (t[:, 0] - 0.5) * -1 + 0.5
        t = t.reshape(p.shape)
    if kind == "row_norm":
        d = (p - t).reshape(-1, 3)
        e32 = sqrt_rn((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        e64 = torch.linalg.norm(d.double(), dim=1)
        return float(e32.double().sum()), float(e64.sum())
    if kind == "l2":
        d = p - t
        return float((d * d).double().sum()), float(F.mse_loss(p.double(), t.double(), reduction="sum"))
    if kind == "smooth_l1":
        z = (p - t).abs()
        e32 = torch.where(z < 1, 0.5 * z * z, z - 0.5)
        return float(e32.double().sum()), float(F.smooth_l1_loss(p.double(), t.double(), reduction="sum", beta=1.0))
    e32 = torch.clamp(p, min=0) - p * t + torch.log1p(torch.exp(-p.abs()))
    return float(e32.double().sum()), float(F.binary_cross_entropy_with_logits(p.double(), t.double(), reduction="sum"))


def value_inputs(kind, m, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(m, 3, generator=g)
    if kind == "bce_logits":
        t = (t > 0.5).float()
        p = torch.randn(m, 3, generator=g) * 25                          # |x| > 30 in the tail
        p[:7] = torch.tensor([[35.0, -35.0, 0.0], [-40, 40, 1e-3]] * 3 + [[80.0, -80.0, 31.0]])[:m]
    elif kind == "smooth_l1":
        p = t + torch.randn(m, 3, generator=g) * 1.0                     # |d| around 1
        p[:3] = t[:3] + torch.tensor([[1.0, -1.0, 0.999999], [1.000001, -0.5, 2.0], [0.0, 3.0, -1.0]])[:m]
    else:
        p = t + torch.randn(m, 3, generator=g) * 0.3
    return p.to(DEV), t.to(DEV)


@pytest.mark.parametrize("kind", ["l2", "smooth_l1", "bce_logits", "row_norm"])
@pytest.mark.parametrize("m", [1, 1000, 24 * 6000])
def test_value_losses_against_restatements(kind, m):
    p, t = value_inputs(kind, m, seed=m + len(kind))
    out = ops.value_losses([(p, t, kind, True), (p, t, kind)]).cpu().numpy()
    want32, want64 = value_restatement(p, t, kind, False)
    m32, m64 = value_restatement(p, t, kind, True)
    for got, w32, w64 in ((out[0, 0], want32, want64), (out[0, 1], m32, m64), (out[1, 0], want32, want64)):
        assert rel(got, w32) <= 1e-9, (got, w32)
        assert rel(got, w64) <= 1e-6, (got, w64)
    assert out[1, 1] == 0.0


def test_value_losses_one_launch_for_a_batch_and_bits():
    """volume (B, M), surface (B, M, 3), mc surface (B, M, 1) of the reference's validation shape in one launch; identical bits twice"""
    g = torch.Generator().manual_seed(3)
    pv, gv = torch.randn(24, 6000, generator=g).to(DEV), torch.rand(24, 6000, generator=g).to(DEV)
    ps, gs = torch.randn(24, 6000, 3, generator=g).to(DEV), torch.randn(24, 6000, 3, generator=g).to(DEV)
    pm, gm = torch.randn(24, 6000, 1, generator=g).to(DEV) * 40, (torch.rand(24, 6000, 1, generator=g) > 0.5).float().to(DEV)
    segs = [(pv, gv, "l2"), (ps, gs, "smooth_l1"), (pm, gm, "bce_logits")]
    a, b = ops.value_losses(segs), ops.value_losses(segs)
    assert torch.equal(a, b)
    for k, (p, t, kind) in enumerate(segs):
        assert rel(float(a[k, 0]), value_restatement(p, t, kind, False)[1]) <= 1e-6


# ------------------------------------------------------------------------------------------------ the reference's metric dicts
def _gold():
    return np.load(GOLDEN)


@pytest.mark.parametrize("ci", range(6))
def test_pointnet2_metrics_reproduce_reference(ci):
    g = _gold()
    p = f"p{ci}/"
    bins, sym, wn, wg = g[p + "params"]
    bins = None if np.isnan(bins) else int(bins)
    sym = None if np.isnan(sym) else int(sym)
    hp = dict(S.default_hparams()["pointnet2_params"], nocs_bins=bins, symmetry_axis=sym)
    model = PointNet2NOCS(nocs_loss_weight=float(wn), grip_point_loss_weight=float(wg), **hp)
    d = {k: torch.from_numpy(g[p + k]).to(DEV) for k in ("logits", "global_logits", "y", "nocs_grip_point")}
    batch = type("B", (), {"y": d["y"], "nocs_grip_point": d["nocs_grip_point"]})()
    got = model.validation_metrics(batch, result={"per_point_logits": d["logits"], "global_logits": d["global_logits"]})
    want = {k[len(p + "metric/"):]: float(g[k]) for k in g.files if k.startswith(p + "metric/")}
    assert set(got) == set(want)
    for k in want:
        assert rel(got[k], want[k]) <= 1e-6, (k, got[k], want[k])
    if p + "mirrored_chosen" in g.files:       # the batch-level choice: the chosen branch's nocs_loss, not a per-point mix
        assert bool(g[p + "mirrored_chosen"]) == (ci in (4, 5))


@pytest.mark.parametrize("ci", range(3))
def test_pipeline_losses_reproduce_reference(ci):
    g = _gold()
    p = f"w{ci}/"
    lt, cls, wv, ws, wm = g[p + "params"]
    hp = S.default_hparams(grid=8, mc_surface=wm > 0)
    model = ConvImplicitWNFPipeline(**{**hp, "mc_surface_loss_weight": float(wm)}, loss_type=["l2", "smooth_l1"][int(lt)],
                                    volume_classification=bool(cls), volume_loss_weight=float(wv), surface_loss_weight=float(ws))
    t = {k: torch.from_numpy(g[p + k]).to(DEV) for k in ("pred_volume_value", "gt_volume_value", "pred_sim_points", "gt_sim_points", "pred_mc",
                                                         "is_query_point_on_surf")}
    result = {"volume_decoder_result": {"pred_volume_value": t["pred_volume_value"]}, "surface_decoder_result": {"out_features": t["pred_sim_points"]},
              "mc_surface_decoder_result": {"out_features": t["pred_mc"]}}
    data = type("D", (), {"gt_volume_value": t["gt_volume_value"], "gt_sim_points": t["gt_sim_points"],
                          "is_query_point_on_surf": t["is_query_point_on_surf"]})()
    got = model.losses_from(result, data)
    want = {k[len(p + "metric/"):]: float(g[k]) for k in g.files if k.startswith(p + "metric/")}
    assert set(got) == set(want)
    for k in want:
        assert rel(got[k], want[k]) <= 1e-6, (k, got[k], want[k])


# ------------------------------------------------------------------------------------------------ end to end
def read_csv(path):
    with open(path) as f:
        return [{k: float(v) for k, v in r.items()} for r in csv.DictReader(f)]


def bce32(x, y):
    """BCE-with-logits per element in fp32: max(x, 0) - x * y + log1p(exp(-|x|))"""
    return torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))


def reference_pipeline_losses(model, result, data, fp64_terms):
    """the reference's infer (conv_implicit_wnf.py:405-452) over the decoder outputs and targets, reduced in fp64; the per-element terms
    are torch's own fp32 ones (reduction='none'; BCE in the formula above) or, with fp64_terms, computed in fp64 from the fp32 values"""
    if fp64_terms:
        crit = {"l2": F.mse_loss, "smooth_l1": F.smooth_l1_loss}[model.loss_type]
        bce = F.binary_cross_entropy_with_logits
        cast = torch.Tensor.double
    else:
        fn = {"l2": F.mse_loss, "smooth_l1": F.smooth_l1_loss}[model.loss_type]
        crit = lambda p, t: fn(p, t, reduction="none").double().mean()        # noqa: E731
        bce = lambda p, t: bce32(p, t).double().mean()                        # noqa: E731
        cast = torch.Tensor.float
    pv = cast(result["volume_decoder_result"]["pred_volume_value"])
    vol_crit = bce if model.volume_classification else crit
    out = {"volume_loss": model.volume_loss_weight * float(vol_crit(pv, cast(data.gt_volume_value))),
           "surface_loss": model.surface_loss_weight * float(crit(cast(result["surface_decoder_result"]["out_features"]), cast(data.gt_sim_points)))}
    if model.mc_surface_loss_weight > 0:
        out["mc_surface_loss"] = model.mc_surface_loss_weight * float(bce(cast(result["mc_surface_decoder_result"]["out_features"]),
                                                                          cast(data.is_query_point_on_surf)))
    out["loss"] = sum(out.values())
    return out


def test_validate_main_pipeline_end_to_end(tmp_path):
    store, out_dir = tmp_path / "ds.zarr", tmp_path / "out"
    write_validation_store(str(store), 24)
    argv = ["--model", "pipeline", "--zarr_in", str(store), "--output_dir", str(out_dir), "--subset", "train", "--static_epoch_seed", "--batch_size", "3",
            "--num_batches", "2", "--num_pc_sample", "1000", "--num_volume_sample", "300", "--num_surface_sample", "200",
            "--num_mc_surface_sample", "100", "--volume_size", "12", "--grid", "16", "--mc_surface"]
    summary = V.main(argv)
    rows = read_csv(out_dir / "val_metrics.csv")
    assert len(rows) == 2 and [r["garments"] for r in rows] == [3, 3]
    keys = {"val_volume_loss", "val_surface_loss", "val_mc_surface_loss", "val_loss"}
    assert keys <= set(rows[0])
    saved = json.load(open(out_dir / "summary.json"))
    assert saved["batches"] == 2 and saved["wall_seconds"] > 0 and set(saved["epoch"]) == keys
    for k in keys:
        assert rel(saved["epoch"][k], np.mean([r[k] for r in rows])) <= 1e-12
    assert summary["epoch"] == saved["epoch"]
    a = V.build_parser().parse_args(argv)
    model = V.load_model(a, torch.device(DEV))
    ds = V.make_dataset(a)
    hp = S.default_hparams(grid=16, reduce_method="max", mc_surface=True)
    sd = S.synthetic_state_dict(hp, 0)
    for r, (_, batch) in zip(rows, V.host_batches(ds, ds.subset_indices("train"), 3)):
        data = batch.to(DEV)
        with torch.no_grad():
            res = model(data)
        want = reference_pipeline_losses(model, res, data, fp64_terms=False)
        want64 = reference_pipeline_losses(model, res, data, fp64_terms=True)
        got = model.losses_from(res, data)                               # the kernel over THIS forward's outputs
        for k, w in want.items():
            assert rel(got[k], w) <= 1e-9, (k, got[k], w)
            assert rel(got[k], want64[k]) <= 1e-6, (k, got[k], want64[k])
            assert rel(r["val_" + k], w) <= 1e-5, (k, r["val_" + k], w)  # main()'s own forward (GroupNorm statistics sum with atomics)
        vol = res["unet3d_result"]["out_feature_volume"].cpu().contiguous()
        for name, q, o in (("volume_decoder", data.volume_query_points, res["volume_decoder_result"]["out_features"]),
                           ("surface_decoder", data.surf_query_points, res["surface_decoder_result"]["out_features"]),
                           ("mc_surface_decoder", data.mc_surf_query_points, res["mc_surface_decoder_result"]["out_features"])):
            np.testing.assert_allclose(o.cpu().numpy(), P.implicit_decoder(sd, name, vol, q.cpu()).numpy(), rtol=0, atol=TOL)


def reference_pointnet2_metrics(model, res, data):
    """the reference's get_metrics_bin_simple / _bin_symmetry formulas in fp64 over the model's own logits"""
    bins = model.nocs_bins
    vg = VirtualGrid(grid_shape=(bins,) * 3, batch_size=1, device=res["per_point_logits"].device)

    def branch(axis):
        y, g = mirror(data.y, axis), mirror(data.nocs_grip_point, axis)
        lg = res["per_point_logits"].reshape(-1, bins, 3).double()
        glg = res["global_logits"].reshape(-1, bins, 3).double()
        nocs = float(F.cross_entropy(lg, vg.get_points_grid_idxs(y)))
        grip = float(F.cross_entropy(glg, vg.get_points_grid_idxs(g)))
        pred = vg.idxs_to_points(torch.argmax(res["per_point_logits"].reshape(-1, bins, 3), dim=1)).double()
        gpred = vg.idxs_to_points(torch.argmax(res["global_logits"].reshape(-1, bins, 3), dim=1)).double()
        return {"loss": model.nocs_loss_weight * nocs + model.grip_point_loss_weight * grip, "nocs_loss": nocs, "grip_point_loss": grip,
                "nocs_err_dist": float(torch.linalg.norm(pred - y.double(), dim=-1).mean()),
                "grip_point_err_dist": float(torch.linalg.norm(gpred - g.double(), dim=-1).mean())}

    plain = branch(None)
    if model.symmetry_axis is None:
        return plain
    mirrored = branch(model.symmetry_axis)
    final = dict(plain if plain["loss"] <= mirrored["loss"] else mirrored)
    final["loss"] = min(plain["loss"], mirrored["loss"])
    return final


@pytest.mark.parametrize("symmetry_axis", [None, 0])
def test_validate_main_pointnet2_end_to_end(tmp_path, symmetry_axis):
    store, out_dir = tmp_path / "ds.zarr", tmp_path / "out"
    write_validation_store(str(store), 20)
    hp = S.default_hparams()["pointnet2_params"]
    m = PointNet2NOCS(**{**hp, "symmetry_axis": symmetry_axis})
    m.load_state_dict({k[len("pointnet2_nocs."):]: v for k, v in S.synthetic_state_dict(S.default_hparams(), 4).items()
                       if k.startswith("pointnet2_nocs.")})
    ck = tmp_path / "p2.ckpt"
    m.save_checkpoint(str(ck))
    argv = ["--model", "pointnet2", "--checkpoint_path", str(ck), "--zarr_in", str(store), "--output_dir", str(out_dir), "--subset", "train",
            "--static_epoch_seed", "--batch_size", "4", "--num_batches", "2", "--num_pc_sample", "1500"]
    V.main(argv)
    rows = read_csv(out_dir / "val_metrics.csv")
    keys = {"val_loss", "val_nocs_loss", "val_grip_point_loss", "val_nocs_err_dist", "val_grip_point_err_dist"}
    assert len(rows) == 2 and keys <= set(rows[0])
    a = V.build_parser().parse_args(argv)
    model = V.load_model(a, torch.device(DEV))
    assert model.symmetry_axis == symmetry_axis
    ds = V.make_dataset(a)
    for r, (_, batch) in zip(rows, V.host_batches(ds, ds.subset_indices("train"), 4)):
        data = batch.to(DEV)
        with torch.no_grad():
            res = model(data)
        want = reference_pointnet2_metrics(model, res, data)
        got = model.validation_metrics(data, result=res)
        for k, w in want.items():
            assert rel(got[k], w) <= 1e-6, (k, got[k], w)
            assert rel(r["val_" + k], w) <= 1e-6, (k, r["val_" + k], w)
