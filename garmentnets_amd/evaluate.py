"""GarmentNets evaluation (MI355X-native): the metric stage of the reference's eval.py (eval.py:872-1046) over a prediction.zarr written by
``python -m garmentnets_amd.predict --zarr_out``, without wandb, Hydra, dask or pandas.

    python -m garmentnets_amd.evaluate --prediction prediction.zarr --zarr_in garmentnets_dataset.zarr [--output_dir DIR]

Metrics (common/metrics.py), run in eval.py's order: optimal_gradient_threshold, pc, grip_point, chamfer, hybrid_chamfer, hausdorff
(geodesic is not implemented).  Outputs, as eval.py writes them: summary/metrics/per_sample/{sample_keys, <column>} and
summary/metrics/aggregate/<column> (the nanmean, 0-d float64) into the prediction store; all_metrics.csv, all_metrics_agg.csv (the rows of
pandas' describe) and summary.json into the output directory.

One sample's nearest-neighbour searches of the chamfer and hybrid chamfer metrics go to the GPU as one gn_nearest_neighbor_f64_batch launch,
its Hausdorff searches as one gn_point_mesh_sqdist_batch launch; the gradient-threshold searches of all samples go as one launch before them
(the chamfer metrics read the threshold that metric aggregates).  There is no CPU fallback: tests may pass another ``backend``.

--vis_samples_per_instance N > 0 adds eval.py's visualisation section (eval.py:750-865, 1048-1096) as PNGs instead of wandb 3-D objects: the ranked
selection (vis_selection), then task_mesh_vis, nocs_mesh_vis and nocs_pc_vis of every selected sample under <output_dir>/vis/ (vis_panels,
write_vis; the mesh panels through visualize.render_mesh_batch, the clouds through the point splat).  Without it nothing is rendered.
"""
import argparse
import json
import os
import sys

import numpy as np

from .common import metrics as M
from .io import zarr_store

METRICS = ("optimal_gradient_threshold", "pc", "grip_point", "chamfer", "hybrid_chamfer", "geodesic", "hausdorff")
DEFAULT_METRICS = ("optimal_gradient_threshold", "pc", "chamfer", "hybrid_chamfer")        # eval_default.yaml: eval.<key>.enabled
DEFAULT_THRESHOLD_PATH = "summary/metrics/aggregate/optimal_wnf_gradient_threshold"
DEFAULT_VALUE_KEY = "marching_cubes_mesh/volume_gradient_magnitude"
NULL_KEY = "marching_cubes_mesh/volume_gradient_magnitude"
DESCRIBE_ROWS = ("count", "mean", "std", "min", "25%", "50%", "75%", "max")


def metric_columns(name, predict_holes=True):
    """the columns one metric writes, in eval.py's order"""
    return {"optimal_gradient_threshold": M.THRESHOLD_COLUMNS, "pc": M.PC_COLUMNS, "grip_point": M.grip_point_columns(),
            "chamfer": M.chamfer_columns(predict_holes), "hybrid_chamfer": M.hybrid_chamfer_columns(predict_holes),
            "hausdorff": M.hausdorff_columns(predict_holes)}[name]


def is_null(sample):
    """eval.py:940-949 with null_key = marching_cubes_mesh/volume_gradient_magnitude: missing, empty, or a NaN first element (predict's
    placeholder for a garment without a surface)"""
    if NULL_KEY not in sample:
        return True
    arr = np.asarray(sample[NULL_KEY])
    return len(arr) == 0 or bool(np.isnan(arr.flatten()[0]))


def resolve_threshold(root, value):
    """override_all.value_threshold: a number, or a path in the prediction store read AFTER the threshold metric has written its
    aggregate (eval.py:980-982)"""
    if not isinstance(value, str):
        return float(value)
    if value not in root:
        raise KeyError(f"value_threshold: {value!r} is not in the prediction store -- enable optimal_gradient_threshold (it writes "
                       f"{DEFAULT_THRESHOLD_PATH}) or pass a number")
    return float(np.array(root[value]))


def _fmt(v):
    return "" if np.isnan(v) else repr(float(v))


def describe(values):
    """pandas' Series.describe() of a float column: count, mean, std (ddof 1), min, quartiles (linear), max over the non-NaN values"""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    n = len(v)
    if n == 0:
        return [0.0] + [float("nan")] * 7
    q = np.percentile(v, [25, 50, 75])
    return [float(n), float(np.mean(v)), float(np.std(v, ddof=1)) if n > 1 else float("nan"), float(v.min()), float(q[0]), float(q[1]),
            float(q[2]), float(v.max())]


def _nanmean(v):
    v = np.asarray(v)
    ok = ~np.isnan(v)
    return np.mean(v[ok]) if ok.any() else v.dtype.type(np.nan)


def write_outputs(output_dir, columns, table, null):
    """all_metrics.csv, all_metrics_agg.csv, summary.json (eval.py:1034-1040) -> the summary dict"""
    os.makedirs(output_dir, exist_ok=True)
    cols = list(columns) + ["null_percentage"]
    data = [table[c] for c in columns] + [null.astype(np.float32)]
    n = len(null)
    with open(os.path.join(output_dir, "all_metrics.csv"), "w") as f:
        f.write("," + ",".join(cols) + "\n")
        for i in range(n):
            f.write(str(i) + "," + ",".join(_fmt(d[i]) for d in data) + "\n")
    desc = [describe(d) for d in data]
    with open(os.path.join(output_dir, "all_metrics_agg.csv"), "w") as f:
        f.write("," + ",".join(cols) + "\n")
        for r, name in enumerate(DESCRIBE_ROWS):
            f.write(name + "," + ",".join(_fmt(d[r]) for d in desc) + "\n")
    summary = {c: float(_nanmean(d)) for c, d in zip(cols, data)}
    with open(os.path.join(output_dir, "summary.json"), "w") as f:
        json.dump(summary, f, indent=2)
    return summary


# ------------------------------------------------------------------------------------------------ eval.py's visualisation section
VIS_FUNCS = ("task_mesh_vis", "nocs_mesh_vis", "nocs_pc_vis")                               # eval.py:1068-1072, in its order
DEFAULT_RANK_METRIC = "hybrid_chamfer_symmetrical_regular_pred"
VIS_KERNEL_SIZE = 4                                                                         # the point panels' footprint (render_nocs's default)


def vis_selection(rank_values, samples_per_instance, num_normal=10, num_best=2, num_worst=2):
    """eval.py:1054-1066 -> {row: label} for the rows that exist.  The rank column is sorted ascending with NaNs last; best = the first num_best,
    worst = the last num_best reversed -- the reference reads num_best there too and never num_worst (kept: the slip is the reference's, and
    num_best = 0 therefore labels every row "worst"); regular_i = i * samples_per_instance.  Labels are written regular, best, worst, a later one
    replacing an earlier one; a regular row past the end is never looked up.  The sort is stable (pandas' default quicksort is not, so the
    reference's own order among equal rank values is not pinned; here the lower row comes first)."""
    del num_worst
    rank = np.asarray(rank_values, dtype=np.float64)
    order = [int(i) for i in np.argsort(rank, kind="stable")]                               # numpy sorts NaNs last
    best = order[:num_best]
    worst = order[-num_best:][::-1]
    labels = {}
    for i in range(num_normal):
        labels[i * samples_per_instance] = "regular_{0:02d}".format(i)
    for i, row in enumerate(best):
        labels[row] = "best_{0:02d}".format(i)
    for i, row in enumerate(worst):
        labels[row] = "worst_{0:02d}".format(i)
    return {row: labels[row] for row in range(len(rank)) if row in labels}


def _rgba(rgb):
    rgb = np.asarray(rgb, dtype=np.float32).reshape(-1, 3)
    return np.concatenate([rgb, np.ones((len(rgb), 1), np.float32)], axis=1)


def vis_panels(sample, func_key, side, sim_normalizer, value_threshold, value_key=DEFAULT_VALUE_KEY, value_delta=0.1, predict_holes=True,
               volume_task_space=False, null=False):
    """the panels of one eval.py visualisation function seen from `side`, left to right where the wandb object's offsets put them:
    [("mesh", mesh_spec) | ("points", image_spec) | ("blank", None)].  A null sample's predicted mesh panels are blank (background)."""
    from . import visualize as V

    def arr(key, dtype=np.float32):
        return np.asarray(sample[key]).astype(dtype)

    if func_key == "nocs_pc_vis":                     # GT NOCS cloud | predicted NOCS cloud coloured by GT NOCS | the same coloured by confidence
        gt, pred = arr("point_cloud/gt_nocs"), arr("point_cloud/pred_nocs")
        conf = arr("point_cloud/pred_nocs_confidence").reshape(len(pred), -1)
        # the per-axis confidences are the colour, as eval.py has them (confidence * 255 as RGB); a single column goes through viridis
        by_conf = dict(colors=_rgba(conf)) if conf.shape[1] == 3 else dict(values=conf[:, 0].copy(), vrange=V.CONFIDENCE_RANGE)
        return [("points", V.image_spec(gt, side, VIS_KERNEL_SIZE, colors=_rgba(gt))),
                ("points", V.image_spec(pred, side, VIS_KERNEL_SIZE, colors=_rgba(gt))),
                ("points", V.image_spec(pred, side, VIS_KERNEL_SIZE, **by_conf))]
    gt_nocs, gt_faces = arr("gt_mesh/cloth_nocs_verts"), arr("gt_mesh/cloth_faces_tri", np.int32)
    if not null:
        pred_nocs, pred_sim = arr("marching_cubes_mesh/verts"), arr("marching_cubes_mesh/warp_field")
        pred_faces = arr("marching_cubes_mesh/faces", np.int32).reshape(-1, 3)
        if volume_task_space:                         # the volume is in task space: verts are simulation space, the warp field is NOCS
            pred_nocs, pred_sim = pred_sim, pred_nocs
        value = arr(value_key).reshape(-1) if predict_holes else None
    if func_key == "nocs_mesh_vis":                   # GT NOCS mesh | predicted NOCS mesh coloured by its value around the threshold
        panels = [("mesh", V.mesh_spec(gt_nocs, gt_faces, _rgba(gt_nocs), side))]
        if null:
            return panels + [("blank", None)]
        if predict_holes:
            colors = V.viridis(value, value_threshold - value_delta, value_threshold + value_delta)
        else:
            colors = np.ones((len(pred_nocs), 4), dtype=np.float32)
        return panels + [("mesh", V.mesh_spec(pred_nocs, pred_faces, colors, side))]
    if func_key != "task_mesh_vis":
        raise ValueError(f"unknown visualisation {func_key!r}")
    # GT simulation mesh | predicted simulation mesh | the input cloud, all through the dataset's task-space normaliser into the unit cube
    panels = [("mesh", V.mesh_spec(sim_normalizer(arr("gt_mesh/cloth_verts")).astype(np.float32), gt_faces, _rgba(gt_nocs), side))]
    if null:
        panels.append(("blank", None))
    else:
        if predict_holes:                             # eval.py filters vertices; a face stays iff all three of its vertices do (no component step)
            ok = value > value_threshold
            pred_faces = pred_faces[ok[pred_faces].all(axis=1)] if len(pred_faces) else pred_faces
        panels.append(("mesh", V.mesh_spec(sim_normalizer(pred_sim).astype(np.float32), pred_faces, _rgba(pred_nocs), side)))
    cloud = sim_normalizer(arr("point_cloud/input_points")).astype(np.float32)
    return panels + [("points", V.image_spec(cloud, side, VIS_KERNEL_SIZE, colors=_rgba(arr("point_cloud/input_rgb") / np.float32(255))))]


def write_vis(output_dir, samples, null, selection, sim_aabb, sides=("front",), img_size=256, vis_backend="device", **panel_args):
    """<output_dir>/vis/<func_key>_<label>.png for every selected row: the function's panels side by side, one row of them per side.  Every mesh
    panel of the call goes through one launch pair, every point panel through another -> the files written"""
    from . import visualize as V
    from .io.dataset import AABBGripNormalizer
    normalizer = AABBGripNormalizer(np.asarray(sim_aabb))
    S = int(img_size)
    grids, jobs = [], {"mesh": [], "points": []}
    for row, label in selection.items():
        for func_key in VIS_FUNCS:
            grid = []
            for side in sides:
                line = []
                for kind, spec in vis_panels(samples[row], func_key, side, normalizer, null=bool(null[row]), **panel_args):
                    if kind == "points":
                        spec["kernel_size"] = min(spec["kernel_size"], S)
                    if kind != "blank":
                        jobs[kind].append(spec)
                    line.append((kind, len(jobs[kind]) - 1 if kind != "blank" else None))
                grid.append(line)
            grids.append((f"{func_key}_{label}", grid))
    images = {"mesh": V.render_mesh_batch(jobs["mesh"], S, vis_backend), "points": V.render_batch(jobs["points"], S, vis_backend)}
    blank = np.empty((S, S, 4), dtype=np.float32)
    blank[:, :] = np.asarray((1, 1, 1, 0), dtype=np.float32)
    files = []
    for name, grid in grids:
        img = np.concatenate([np.concatenate([blank if kind == "blank" else images[kind][j] for kind, j in line], axis=1) for line in grid], axis=0)
        files.append(os.path.join(output_dir, "vis", name + ".png"))
        V.write_png(files[-1], img)
    return files


def evaluate_store(prediction, nocs_aabb, output_dir=".", metrics=DEFAULT_METRICS, precision_weight=0.75, num_points=10000, seed=0,
                   value_threshold=DEFAULT_THRESHOLD_PATH, value_key=DEFAULT_VALUE_KEY, predict_holes=True, volume_task_space=False, backend=None,
                   verbose=False, vis_samples_per_instance=0, vis_rank_metric=DEFAULT_RANK_METRIC, vis_num_normal=10, vis_num_best=2,
                   vis_num_worst=2, vis_value_delta=0.1, vis_img_size=256, vis_sides=("front",), sim_aabb=None, vis_backend="device"):
    """eval.py's metric stage over the prediction store `prediction` -> dict(sample_keys, columns, table {column: float64 [N]},
    is_null [N] bool, summary, errors [(metric, sample_key, message)]).  vis_samples_per_instance > 0: eval.py's visualisation section after it
    (vis_selection, write_vis; sim_aabb = the dataset's summary/cloth_aabb_union) -> also vis_files"""
    unknown = sorted(set(metrics) - set(METRICS))
    if unknown:
        raise ValueError(f"unknown metrics {unknown}")
    if "geodesic" in metrics:
        raise ValueError("metric 'geodesic' is not implemented (eval.py's potpourri3d heat-method geodesics are out of scope)")
    metrics = [m for m in METRICS if m in set(metrics)]          # eval.py's order, whatever the order asked for
    if vis_samples_per_instance > 0:
        if vis_rank_metric not in [c for m in metrics for c in metric_columns(m, predict_holes)]:
            raise ValueError(f"vis_rank_metric {vis_rank_metric!r} is not a column of the enabled metrics {metrics}")
        if sim_aabb is None:
            raise ValueError("the visualisation needs sim_aabb, the dataset's summary/cloth_aabb_union (--zarr_in)")
    if backend is None:
        backend = M.default_backend()
    nocs_aabb = np.asarray(nocs_aabb)
    root = zarr_store.open_group(prediction, create=False)
    samples_group = root["samples"]
    keys = samples_group.keys()
    samples = [samples_group[k] for k in keys]
    null = np.array([is_null(s) for s in samples], dtype=bool)
    live = [i for i in range(len(keys)) if not null[i]]
    compressor = zarr_store.default_compressor()
    per_sample = root.require_group("summary/metrics/per_sample")
    aggregate = root.require_group("summary/metrics/aggregate")
    per_sample.array("sample_keys", np.array(keys), compressor=compressor)

    columns, table, errors = [], {}, []
    override = dict(value_key=value_key, predict_holes=predict_holes, volume_task_space=volume_task_space)

    def record(name, results):
        """results: {sample index: metric dict or exception} -> the metric's columns (NaN where a sample is null or failed), stored"""
        cols = metric_columns(name, predict_holes)
        for i, r in results.items():
            if isinstance(r, Exception):
                errors.append((name, keys[i], f"{type(r).__name__}: {r}"))
        for c in cols:
            v = np.full(len(keys), np.nan)
            for i, r in results.items():
                if isinstance(r, dict) and c in r:
                    v[i] = float(r[c])
            columns.append(c)
            table[c] = v
            per_sample.array(c, v, compressor=compressor)
            aggregate.array(c, np.array(_nanmean(v), dtype=np.float64), compressor=compressor)
        if verbose:
            print(json.dumps({"metric": name, "errors": sum(isinstance(r, Exception) for r in results.values())}), flush=True)

    def host(fn, **kw):
        out = {}
        for i in live:
            try:
                with np.errstate(all="ignore"):
                    out[i] = fn(samples[i], **kw)
            except Exception as e:      # noqa: BLE001 -- the reference's parallel_map: one (metric, sample) fails alone
                out[i] = e
        return out

    def planned(make, batches):
        """plans of `make` per live sample; batches: 'all' = every sample's searches in one backend call, 'sample' = one call per sample"""
        plans = {}
        for i in live:
            try:
                plans[i] = make(samples[i])
            except Exception as e:      # noqa: BLE001
                plans[i] = e
        ok = [i for i in live if not isinstance(plans[i], Exception)]
        out = dict(plans)
        groups = [ok] if batches == "all" else [[i] for i in ok]
        for g in groups:
            out.update(zip(g, run_isolated([plans[i] for i in g])))
        return out

    def run_isolated(plans):
        """run_plans with the searches of all `plans` in one backend call; when that call raises, each plan again in a call of its own, so
        that one sample's (or one metric's) bad input fails that (metric, sample) alone"""
        try:
            return M.run_plans(plans, backend)
        except Exception as e:          # noqa: BLE001
            if len(plans) == 1:
                return [e]
        return [r for pl in plans for r in run_isolated([pl])]

    if "optimal_gradient_threshold" in metrics:
        record("optimal_gradient_threshold", planned(lambda s: M.plan_optimal_gradient_threshold(s, precision_weight=precision_weight), "all"))
    if "pc" in metrics:
        record("pc", host(M.pc_metrics, nocs_aabb=nocs_aabb))
    # eval.py:984-988: every enabled function but the threshold and pc gets the override set, a value_threshold path dereferenced when the
    # function's turn comes -- after the threshold function has written its aggregate (grip_point reads none of it, but fails the same way)
    if any(m in metrics for m in ("grip_point", "chamfer", "hybrid_chamfer", "hausdorff")):
        override["value_threshold"] = resolve_threshold(root, value_threshold)
    if "grip_point" in metrics:
        record("grip_point", host(M.grip_point_metrics, nocs_aabb=nocs_aabb, **override))
    rest = [m for m in ("chamfer", "hybrid_chamfer", "hausdorff") if m in metrics]
    if rest:
        kw = dict(nocs_aabb=nocs_aabb, num_points=num_points, seed=seed, **override)
        # chamfer + hybrid chamfer: one nearest-neighbour launch per sample
        makers = {"chamfer": lambda s: M.plan_sampled_chamfer(s, **kw), "hybrid_chamfer": lambda s: M.plan_sampled_hybrid_chamfer(s, **kw)}
        nn_metrics = [m for m in ("chamfer", "hybrid_chamfer") if m in metrics]
        results = {m: {} for m in nn_metrics}
        for i in live:
            plans = {}
            for m in nn_metrics:
                try:
                    plans[m] = makers[m](samples[i])
                except Exception as e:  # noqa: BLE001
                    results[m][i] = e
            for m, r in zip(plans, run_isolated(list(plans.values()))):
                results[m][i] = r
        for m in nn_metrics:
            record(m, results[m])
        if "hausdorff" in metrics:
            record("hausdorff", planned(lambda s: M.plan_hausdorff(s, backend=backend, **{k: v for k, v in kw.items()
                                                                                          if k not in ("num_points", "seed")}), "sample"))

    summary = write_outputs(output_dir, columns, table, null)
    out = dict(sample_keys=keys, columns=columns, table=table, is_null=null, summary=summary, errors=errors)
    if vis_samples_per_instance > 0:                             # eval.py:1048-1096; the override set and its dereference are the metrics'
        selection = vis_selection(table[vis_rank_metric], vis_samples_per_instance, vis_num_normal, vis_num_best, vis_num_worst)
        out["vis_files"] = write_vis(output_dir, samples, null, selection, sim_aabb, sides=tuple(vis_sides), img_size=vis_img_size,
                                     vis_backend=vis_backend, value_threshold=resolve_threshold(root, value_threshold), value_key=value_key,
                                     value_delta=vis_value_delta, predict_holes=predict_holes, volume_task_space=volume_task_space)
    return out


def _threshold_arg(s):
    try:
        return float(s)
    except ValueError:
        return s


def build_parser():
    ap = argparse.ArgumentParser(description="GarmentNets evaluation (MI355X-native): eval.py's metrics over a prediction.zarr")
    ap.add_argument("--prediction", required=True, help="the prediction.zarr directory (predict --zarr_out)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--zarr_in", help="the dataset store: nocs_aabb = summary/cloth_canonical_aabb_union, in its stored dtype")
    src.add_argument("--nocs_aabb", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"), help="the NOCS AABB (float64)")
    ap.add_argument("--output_dir", default=".", help="where all_metrics.csv, all_metrics_agg.csv and summary.json go (default: .)")
    ap.add_argument("--metrics", nargs="+", default=list(DEFAULT_METRICS), choices=METRICS,
                    help="enabled metrics (eval.<compute_*>.enabled; default: %(default)s)")
    ap.add_argument("--precision_weight", type=float, default=0.75, help="eval.compute_optimal_gradient_treshold.precision_weight")
    ap.add_argument("--num_points", type=int, default=10000, help="eval.compute_(hybrid_)chamfer.num_points")
    ap.add_argument("--seed", type=int, default=0, help="eval.compute_(hybrid_)chamfer.seed")
    ap.add_argument("--value_threshold", type=_threshold_arg, default=DEFAULT_THRESHOLD_PATH,
                    help="override_all.value_threshold: a number or a path in the prediction store (default: %(default)s)")
    ap.add_argument("--value_key", default=DEFAULT_VALUE_KEY, help="override_all.value_key")
    ap.add_argument("--predict_holes", dest="predict_holes", action="store_true", default=True, help="override_all.predict_holes (default)")
    ap.add_argument("--no_predict_holes", dest="predict_holes", action="store_false", help="override_all.predict_holes = False")
    ap.add_argument("--volume_task_space", action="store_true", help="override_all.volume_task_space")
    ap.add_argument("--vis_samples_per_instance", type=int, default=0,
                    help="vis.samples_per_instance: > 0 writes <output_dir>/vis/<function>_<label>.png for the ranked selection (needs --zarr_in); "
                         "0 (eval_default.yaml): nothing is rendered")
    ap.add_argument("--vis_rank_metric", default=DEFAULT_RANK_METRIC, help="vis.rank_metric: a column of the enabled metrics (default: %(default)s)")
    ap.add_argument("--vis_num_normal", type=int, default=10, help="vis.num_normal")
    ap.add_argument("--vis_num_best", type=int, default=2, help="vis.num_best (eval.py sizes the worst list by it too)")
    ap.add_argument("--vis_num_worst", type=int, default=2, help="vis.num_worst (eval.py never reads it)")
    ap.add_argument("--vis_value_delta", type=float, default=0.1, help="vis.nocs_mesh_vis.value_delta")
    ap.add_argument("--vis_img_size", type=int, default=256, help="the side of one panel in pixels")
    ap.add_argument("--vis_sides", nargs="+", default=["front"], choices=("front", "top", "left"), help="one row of panels per side")
    return ap


def main(argv=None, backend=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if "geodesic" in a.metrics:
        ap.error("--metrics geodesic: not implemented (the heat-method geodesics of eval.py's compute_geodesic are out of scope)")
    sim_aabb = None
    if a.vis_samples_per_instance > 0 and not a.zarr_in:
        ap.error("--vis_samples_per_instance: the task-space panels need the dataset's cloth_aabb_union, pass --zarr_in")
    if a.zarr_in:
        summary = zarr_store.open_group(a.zarr_in, create=False)["summary"]
        nocs_aabb = summary["cloth_canonical_aabb_union"]
        if a.vis_samples_per_instance > 0:
            sim_aabb = np.asarray(summary["cloth_aabb_union"])
    else:
        nocs_aabb = np.array(a.nocs_aabb, dtype=np.float64).reshape(2, 3)
    out = evaluate_store(a.prediction, nocs_aabb, output_dir=a.output_dir, metrics=a.metrics, precision_weight=a.precision_weight,
                         num_points=a.num_points, seed=a.seed, value_threshold=a.value_threshold, value_key=a.value_key,
                         predict_holes=a.predict_holes, volume_task_space=a.volume_task_space, backend=backend, verbose=True,
                         vis_samples_per_instance=a.vis_samples_per_instance, vis_rank_metric=a.vis_rank_metric, vis_num_normal=a.vis_num_normal,
                         vis_num_best=a.vis_num_best, vis_num_worst=a.vis_num_worst, vis_value_delta=a.vis_value_delta,
                         vis_img_size=a.vis_img_size, vis_sides=a.vis_sides, sim_aabb=sim_aabb)
    for name, key, msg in out["errors"]:
        print(f"error: {name} {key}: {msg}", file=sys.stderr)
    print(json.dumps(out["summary"], indent=2))
    return out


if __name__ == "__main__":
    main()
