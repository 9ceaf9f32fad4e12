#!/usr/bin/env python3
"""Golden vectors for validation (targets and losses) from the REFERENCE's own code (build container only).

Run:  python tests/golden/make_golden_validate.py       (needs /root/reference; never runs on the GPU box)

The reference's dataset (datasets/conv_implicit_wnf_dataset.py) and its two Lightning modules are imported with make_golden_ref's stubs;
igl.doublearea is stubbed by an independent numpy formula (|cross(v1 - v0, v2 - v0)|), so libigl's own area arithmetic is not pinned here.
Unmodified reference methods run on synthetic data bound to bare objects carrying the attributes their __init__ would have set:
  data_io + get_volume_sample / get_surface_sample / get_mc_surface_sample + the __getitem__ order (noise, rotation)   -> d<case>/...
  PointNet2NOCS.get_metrics_regression / _bin_simple / _bin_symmetry                                                  -> p<case>/...
  ConvImplicitWNFPipeline.infer on given decoder outputs                                                               -> w<case>/...
Only DATA (inputs, parameters, outputs) is written to ref_validate.npz.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_dataset as GD  # noqa: E402
import make_golden_ref as G  # noqa: E402


def np_doublearea(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces)
    return np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)


class FakeGroup(dict):
    """a zarr group as data_io reads it: nested dicts of numpy arrays plus .attrs.asdict()"""

    def __init__(self, attrs=None, **kw):
        super().__init__(**kw)
        self.attrs = types.SimpleNamespace(asdict=lambda: dict(attrs or {}))


def sample_group(sample, volume_group, volume_size, volume, mc):
    return FakeGroup(
        attrs={"scale": sample["scale"], "grip_vertex_idx": sample["grip_vertex_idx"]},
        point_cloud={"nocs": sample["pc_nocs"], "point": sample["pc_sim"], "rgb": sample["pc_sim_rgb"], "sizes": sample["pc_sizes"]},
        mesh={"cloth_verts": sample["cloth_sim_verts"], "cloth_nocs_verts": sample["cloth_nocs_verts"], "cloth_faces_tri": sample["cloth_faces_tri"]},
        volume={volume_group: {str(volume_size): volume}},
        marching_cube_mesh=mc)


DATASET_CASES = [
    dict(idx=3, ratio=0.0, group="nocs_winding_number_field", clip=None, absval=False, rot=True, noise=0.0, mc=True, nvol=300, nsurf=250),
    dict(idx=5, ratio=0.5, group="nocs_occupancy_grid", clip=None, absval=False, rot=False, noise=0.0, mc=True, nvol=301, nsurf=200),
    dict(idx=8, ratio=0.5, group="nocs_signed_distance_field", clip=0.05, absval=True, rot=True, noise=0.01, mc=False, nvol=200, nsurf=180),
    dict(idx=9, ratio=0.25, group="sim_nocs_winding_number_field", clip=None, absval=False, rot=True, noise=0.0, mc=False, nvol=240, nsurf=160),
]


def dataset_cases(Ref, out):
    import pandas as pd
    for ci, c in enumerate(DATASET_CASES):
        rs = np.random.RandomState(500 + ci)
        sample = GD.synthetic_sample(200 + ci)
        vs = 9
        volume = (rs.normal(size=(vs, vs, vs)) * (0.1 if c["clip"] else 1.0)).astype(np.float32)
        if c["group"] == "nocs_occupancy_grid":
            volume = (rs.uniform(size=(vs, vs, vs)) > 0.5).astype(np.float32)
        mc = {"marching_cube_verts": rs.uniform(size=(400, 3)).astype(np.float32),
              "marching_cube_faces": rs.randint(0, 400, size=(700, 3)).astype(np.int32),
              "is_vertex_on_surface": rs.uniform(size=400) > 0.4}
        aabb = np.array([[-0.4, -0.45, -0.9], [0.42, 0.4, 0.05]], dtype=np.float32)
        task = c["group"] == "sim_nocs_winding_number_field"
        grp = sample_group(sample, c["group"], vs, volume, mc)
        self = types.SimpleNamespace(
            groups_df=pd.DataFrame({"group_key": ["k"] * (c["idx"] + 1)}), samples_group={"k": grp}, volume_size=vs, volume_group=c["group"],
            tsdf_clip_value=c["clip"], volume_absolute_value=c["absval"], num_volume_sample=c["nvol"], num_surface_sample=c["nsurf"],
            num_mc_surface_sample=c["nsurf"] if c["mc"] else 0, num_pc_sample=500, static_epoch_seed=True, num_views=4, cloth_sim_aabb=aabb,
            surface_sample_ratio=c["ratio"], surface_sample_std=0.05, surface_normal_noise_ratio=0, surface_normal_std=0,
            volume_task_space=task, pc_noise_std=c["noise"], random_rot_range=(-180, 180), enable_augumentation=c["rot"])
        for name in ("reshape_for_batching",):
            setattr(self, name, types.MethodType(getattr(Ref, name), self))
        data_in = Ref.data_io(self, c["idx"])
        data = Ref.get_base_data(self, c["idx"], data_in=data_in)
        vol = Ref.get_volume_sample(self, c["idx"], data_in=data_in)
        surf = Ref.get_surface_sample(self, c["idx"], data_in=data_in)
        data.update(vol)
        data.update(surf)
        if c["mc"]:
            mcs = Ref.get_mc_surface_sample(self, c["idx"], data_in=data_in)
            data.update(mcs)
        data["input_aug_rot_mat"] = np.expand_dims(np.eye(3, dtype=np.float32), axis=0)
        if c["noise"] > 0:
            data = Ref.noise_augumentation(self, c["idx"], data=data)
        if c["rot"]:
            data = Ref.rotation_augumentation(self, c["idx"], data=data)
        p = f"d{ci}/"
        for k in ("cloth_sim_verts", "cloth_nocs_verts", "cloth_faces_tri"):         # the targets read the meshes only
            out[p + "in/" + k] = sample[k]
        for k, v in mc.items():
            out[p + "in/" + k] = v
        out[p + "in/volume"] = volume
        out[p + "aabb"] = aabb
        out[p + "volume"] = data_in["volume"]
        for k, v in vol.items():
            out[p + "vol/" + k] = v
        for k, v in surf.items():
            out[p + "surf/" + k] = v
        if c["mc"]:
            for k, v in mcs.items():
                out[p + "mc/" + k] = v
        for k in ("volume_query_points", "gt_volume_value", "surf_query_points", "gt_sim_points", "mc_surf_query_points",
                  "is_query_point_on_surf", "input_aug_rot_mat"):
            if k in data:
                out[p + "final/" + k] = np.asarray(data[k])


def logits_case(rs, n, b, bins, peaked_at=None):
    """logits (n, bins*3) with exact ties and magnitudes up to 80; targets on bin edges among uniform ones"""
    lg = rs.normal(size=(n, bins, 3)).astype(np.float32) * 4
    lg[::7] = np.round(lg[::7])                      # exact ties
    lg[3::11] *= 20                                  # |x| up to ~80
    y = rs.uniform(size=(n, 3)).astype(np.float32)
    edges = np.array([0.0, 1.0] + [k / (bins - 1) for k in range(bins)], dtype=np.float32)
    y[::5] = edges[rs.randint(0, len(edges), size=(len(y[::5]), 3))]
    grip = rs.uniform(size=(b, 3)).astype(np.float32)
    glg = rs.normal(size=(b, bins, 3)).astype(np.float32) * 3
    if peaked_at is not None:                        # make the prediction follow the given (mirrored) targets
        for arr, tgt in ((lg, peaked_at[0]), (glg, peaked_at[1])):
            idx = np.clip((tgt * (bins - 1)).astype(np.int64), 0, bins - 1)
            for a in range(3):
                arr[np.arange(len(arr)), idx[:, a], a] += 12
    return lg.reshape(n, bins * 3), glg.reshape(b, bins * 3), y, grip


def mirror(p, axis):
    q = p.copy()
    q[:, axis] = (q[:, axis] - np.float32(0.5)) * np.float32(-1) + np.float32(0.5)
    return q


POINTNET2_CASES = [
    dict(bins=None, sym=None, wn=1.0, wg=1.0),
    dict(bins=None, sym=0, wn=1.0, wg=0.5),
    dict(bins=10, sym=None, wn=1.0, wg=1.0),
    dict(bins=10, sym=0, wn=1.0, wg=1.0, follow="plain"),
    dict(bins=10, sym=0, wn=2.0, wg=0.5, follow="mirror"),
    dict(bins=7, sym=1, wn=1.0, wg=1.0, follow="mirror"),
]


def pointnet2_cases(RefP, out):
    from components.loss import MirrorMSELoss
    for ci, c in enumerate(POINTNET2_CASES):
        rs = np.random.RandomState(700 + ci)
        n, b = 240, 4
        if c["bins"] is None:
            lg = rs.uniform(-0.2, 1.2, size=(n, 3)).astype(np.float32)
            glg = rs.uniform(size=(b, 3)).astype(np.float32)
            y = rs.uniform(size=(n, 3)).astype(np.float32)
            grip = rs.uniform(size=(b, 3)).astype(np.float32)
            if c["sym"] is not None:
                lg[: n // 2] = mirror(y, 0)[: n // 2] + rs.normal(size=(n // 2, 3)).astype(np.float32) * 0.01
        else:
            peaked = None
            y0 = rs.uniform(size=(n, 3)).astype(np.float32)
            g0 = rs.uniform(size=(b, 3)).astype(np.float32)
            if c.get("follow") == "mirror":
                peaked = (mirror(y0, c["sym"]), mirror(g0, c["sym"]))
            elif c.get("follow") == "plain":
                peaked = (y0, g0)
            lg, glg, y, grip = logits_case(rs, n, b, c["bins"], peaked)
            if peaked is not None:
                y, grip = y0, g0
        batch_idx = np.repeat(np.arange(b), n // b)
        self = types.SimpleNamespace(nocs_bins=c["bins"], symmetry_axis=c["sym"], nocs_loss_weight=c["wn"], grip_point_loss_weight=c["wg"],
                                     device=torch.device("cpu"),
                                     criterion=torch.nn.MSELoss() if c["sym"] is None else MirrorMSELoss())
        for name in ("get_virtual_grid", "get_metrics_bin_symmetry_helper"):
            setattr(self, name, types.MethodType(getattr(RefP, name), self))
        result = {"per_point_logits": torch.from_numpy(lg), "global_logits": torch.from_numpy(glg),
                  "per_point_features": torch.zeros(n, 4), "per_point_batch_idx": torch.from_numpy(batch_idx)}
        batch = G.StubBatch(y=torch.from_numpy(y), nocs_grip_point=torch.from_numpy(grip), batch=torch.from_numpy(batch_idx))
        if c["bins"] is None:
            metrics, _ = RefP.get_metrics_regression(self, result, batch)
        elif c["sym"] is None:
            metrics, _ = RefP.get_metrics_bin_simple(self, result, batch)
        else:
            metrics, _ = RefP.get_metrics_bin_symmetry(self, result, batch)
            nm, _ = RefP.get_metrics_bin_symmetry_helper(self, result, batch, mirror_axis=None)
            mm, _ = RefP.get_metrics_bin_symmetry_helper(self, result, batch, mirror_axis=c["sym"])
            out[f"p{ci}/mirrored_chosen"] = np.array(bool(mm["loss"] < nm["loss"]))
        p = f"p{ci}/"
        out[p + "params"] = np.array([np.nan if c["bins"] is None else c["bins"], np.nan if c["sym"] is None else c["sym"], c["wn"], c["wg"]])
        out[p + "logits"], out[p + "global_logits"], out[p + "y"], out[p + "nocs_grip_point"] = lg, glg, y, grip
        for k, v in metrics.items():
            out[p + "metric/" + k] = np.array(float(v))


PIPELINE_CASES = [
    dict(loss_type="l2", cls=False, wv=1.0, ws=1.0, wm=0.5),
    dict(loss_type="smooth_l1", cls=True, wv=2.0, ws=0.5, wm=0.0),
    dict(loss_type="smooth_l1", cls=False, wv=1.0, ws=1.0, wm=1.0),
]


class FakePipeline:
    def __init__(self, result, **kw):
        self.__dict__.update(kw)
        self._result = result
        self.logger = types.SimpleNamespace(log_metrics=lambda *a, **k: None)
        self.global_step = 0

    def __call__(self, batch):
        return self._result

    def log(self, *a, **k):
        pass

    def vis_batch(self, *a, **k):
        return {}


def pipeline_cases(RefW, out):
    for ci, c in enumerate(PIPELINE_CASES):
        rs = np.random.RandomState(800 + ci)
        B, M = 3, 200
        gv = rs.uniform(size=(B, M)).astype(np.float32)
        pv = gv + rs.normal(size=(B, M)).astype(np.float32) * rs.choice([0.1, 1.0, 3.0], size=(B, M)).astype(np.float32)
        if c["cls"]:
            gv = (gv > 0.5).astype(np.float32)
            pv = rs.normal(size=(B, M)).astype(np.float32) * 20                      # |x| > 30 in the tail
        gs = rs.normal(size=(B, M, 3)).astype(np.float32)
        ps = gs + rs.normal(size=(B, M, 3)).astype(np.float32) * 0.9                 # |d| around 1 for smooth_l1
        gm = (rs.uniform(size=(B, M, 1)) > 0.5).astype(np.float32)
        pm = rs.normal(size=(B, M, 1)).astype(np.float32) * 35
        result = {"volume_decoder_result": {"pred_volume_value": torch.from_numpy(pv)}, "surface_decoder_result": {"out_features": torch.from_numpy(ps)},
                  "mc_surface_decoder_result": {"out_features": torch.from_numpy(pm)}}
        crit = torch.nn.MSELoss() if c["loss_type"] == "l2" else torch.nn.SmoothL1Loss()
        fake = FakePipeline(result, volume_loss_weight=c["wv"], surface_loss_weight=c["ws"], mc_surface_loss_weight=c["wm"],
                            volume_classification=c["cls"], criterion=crit, binary_criterion=torch.nn.BCEWithLogitsLoss())
        batch = G.StubBatch(gt_volume_value=torch.from_numpy(gv), gt_sim_points=torch.from_numpy(gs), is_query_point_on_surf=torch.from_numpy(gm))
        metrics = RefW.infer(fake, batch, 0, is_train=False)
        p = f"w{ci}/"
        out[p + "params"] = np.array([["l2", "smooth_l1"].index(c["loss_type"]), float(c["cls"]), c["wv"], c["ws"], c["wm"]])
        out[p + "pred_volume_value"], out[p + "gt_volume_value"] = pv, gv
        out[p + "pred_sim_points"], out[p + "gt_sim_points"] = ps, gs
        out[p + "pred_mc"], out[p + "is_query_point_on_surf"] = pm, gm
        for k, v in metrics.items():
            out[p + "metric/" + k] = np.array(float(v))


def main():
    G.install_stubs()
    sys.modules["zarr"] = types.ModuleType("zarr")
    igl = types.ModuleType("igl")
    igl.doublearea = np_doublearea
    sys.modules["igl"] = igl
    vis = types.ModuleType("common.visualization_util")
    vis.get_vis_idxs = vis.render_nocs_pair = vis.render_wnf_pair = vis.render_wnf_points_pair = vis.render_confidence_pair = None
    sys.modules["common.visualization_util"] = vis
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_conv_implicit_wnf_dataset", os.path.join(G.REF, "datasets", "conv_implicit_wnf_dataset.py"))
    ref_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_mod)
    from networks.conv_implicit_wnf import ConvImplicitWNFPipeline as RefW
    from networks.pointnet2_nocs import PointNet2NOCS as RefP
    out = {}
    dataset_cases(ref_mod.ConvImplicitWNFDataset, out)
    pointnet2_cases(RefP, out)
    pipeline_cases(RefW, out)
    path = os.path.join(HERE, "ref_validate.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
