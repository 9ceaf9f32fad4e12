"""CPU: the host logic of the evaluation stage (garmentnets_amd.evaluate, common/metrics.py's eval.py metrics) through the backend hook,
with scipy's cKDTree and a numpy brute-force point-to-triangle distance standing in for the fp64 kernels of csrc/eval_dist.hip."""
import json
import os

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

from garmentnets_amd import evaluate as E
from garmentnets_amd.common import metrics as M
from garmentnets_amd.io import zarr_store


# ------------------------------------------------------------------------------------------------ the CPU backend
def closest_point_sqdist(p, a, b, c):
    """squared distance from every point p (n,3) to every triangle (a, b, c) (m,3 each) -> (n, m), fp64: Ericson's region method
    (Real-Time Collision Detection 5.1.5), evaluated for all regions and selected with masks; degenerate triangles (zero area) are
    measured as their three edges"""
    p = p[:, None, :]
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = np.sum(ab * ap, -1), np.sum(ac * ap, -1)
    bp = p - b
    d3, d4 = np.sum(ab * bp, -1), np.sum(ac * bp, -1)
    cp = p - c
    d5, d6 = np.sum(ab * cp, -1), np.sum(ac * cp, -1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        denom = 1.0 / (va + vb + vc)
        v_in, w_in = vb * denom, vc * denom
        closest = a + ab * v_in[..., None] + ac * w_in[..., None]
        t_ab = d1 / (d1 - d3)
        t_ac = d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    sel = [((d1 <= 0) & (d2 <= 0), np.broadcast_to(a, closest.shape)),
           ((d3 >= 0) & (d4 <= d3), np.broadcast_to(b, closest.shape)),
           ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * t_ab[..., None]),
           ((d6 >= 0) & (d5 <= d6), np.broadcast_to(c, closest.shape)),
           ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * t_ac[..., None]),
           ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + (c - b) * t_bc[..., None])]
    out = closest.copy()
    done = np.zeros(out.shape[:2], dtype=bool)
    for m, q in sel:
        m = m & ~done
        out[m] = q[m]
        done |= m
    d = np.sum((p - out) ** 2, -1)
    seg = np.minimum(np.minimum(_seg_sqdist(p, a, b), _seg_sqdist(p, a, c)), _seg_sqdist(p, b, c))
    degenerate = np.broadcast_to(np.sum(np.cross(ab, ac) ** 2, -1) == 0, d.shape)
    return np.where(degenerate, seg, d)


def _seg_sqdist(p, a, b):
    ab = b - a
    l2 = np.sum(ab * ab, -1)
    with np.errstate(all="ignore"):
        t = np.clip(np.where(l2 > 0, np.sum((p - a) * ab, -1) / l2, 0.0), 0, 1)
    return np.sum((p - (a + ab * t[..., None])) ** 2, -1)


class CpuBackend:
    """scipy / numpy stand-in for metrics.DeviceBackend (same interface, same empty-set conventions as scipy 1.15)"""

    def __init__(self):
        self.nn_calls, self.pm_calls = [], []

    def nearest_neighbor(self, pairs):
        self.nn_calls.append(len(pairs))
        out = []
        for q, r in pairs:
            q, r = np.asarray(q, np.float64), np.asarray(r, np.float64)
            for a in (q, r):
                if a.ndim != 2 or a.shape[1] != 3:       # what ops.nearest_neighbor_f64_batch raises
                    raise ValueError(f"expected an (N, 3) array, got {a.shape}")
            _, idx = cKDTree(r).query(q, k=1)
            if len(r) == 0:
                out.append((idx, np.full(len(q), np.inf)))
                continue
            d = q - r[idx]
            out.append((idx, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))     # cKDTree's order: sqrt(d2) == its distance
        return out

    def point_mesh_sqdist(self, pairs):
        self.pm_calls.append(len(pairs))
        out = []
        for q, v, f in pairs:
            q, v, f = np.asarray(q, np.float64), np.asarray(v, np.float64), np.asarray(f)
            if len(f) == 0:
                out.append((np.full(len(q), -1), np.full(len(q), np.inf)))
                continue
            d = closest_point_sqdist(q, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
            out.append((np.argmin(d, axis=1), np.min(d, axis=1)))
        return out

    def largest_connected_component(self, faces, num_verts):
        if len(faces) == 0:
            raise ValueError("attempt to get argmax of an empty sequence")
        i = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2]])
        j = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0]])
        _, lab = connected_components(coo_matrix((np.ones(len(i)), (i, j)), shape=(num_verts, num_verts)), directed=False)
        return lab == np.argmax(np.bincount(lab))


# ------------------------------------------------------------------------------------------------ a small prediction store
def sheet(n, rng, z=0.0, amp=0.05):
    """a triangulated n x n height field over [0, 1]^2 (a real surface, two triangles per cell) -> verts float32, faces int32"""
    g = np.linspace(0.0, 1.0, n)
    x, y = np.meshgrid(g, g, indexing="ij")
    h = z + amp * np.sin(3 * x + 1) * np.cos(2 * y) + 0.002 * rng.standard_normal(x.shape)
    verts = np.stack([x, y, h], -1).reshape(-1, 3).astype(np.float32)
    k = np.arange(n * n).reshape(n, n)
    a, b, c, d = k[:-1, :-1].ravel(), k[1:, :-1].ravel(), k[1:, 1:].ravel(), k[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    return verts, faces


def write_prediction_sample(samples, key, rng, n=9):
    """one sample with every array eval.py reads: a predicted sheet slightly off the ground-truth one"""
    pv, pf = sheet(n, rng, z=0.02)
    gv, gf = sheet(n + 2, rng)
    mv, mf = sheet(n + 1, rng, z=0.01)
    g = samples.require_group(key)
    mc = g.require_group("marching_cubes_mesh")
    mc.array("verts", pv.astype(np.float64))
    mc.array("faces", pf)
    mc.array("warp_field", (pv * 1.5 + 0.1).astype(np.float32))
    mc.array("volume_gradient_magnitude", rng.random(len(pv)).astype(np.float32))
    pc = g.require_group("point_cloud")
    gt_nocs = rng.random((50, 3)).astype(np.float32)
    pc.array("gt_nocs", gt_nocs)
    pc.array("pred_nocs", (gt_nocs + 0.05 * rng.standard_normal((50, 3))).astype(np.float32))
    misc = g.require_group("misc")
    for k in ("gt_nocs_grip_point", "pred_nocs_grip_point", "pred_global_nocs_grip_point"):
        misc.array(k, rng.random(3).astype(np.float32))
    gm = g.require_group("gt_mesh")
    gm.array("cloth_verts", (gv * 1.5 + 0.1).astype(np.float32))
    gm.array("cloth_nocs_verts", gv)
    gm.array("cloth_faces_tri", gf)
    gmc = g.require_group("gt_marching_cubes_mesh")
    gmc.array("marching_cube_verts", mv)
    gmc.array("marching_cube_faces", mf)
    on = np.ones(len(mv), dtype=bool)
    on[:3] = False
    gmc.array("is_vertex_on_surface", on)
    return g


AABB = np.array([[-0.4, -0.5, -0.3], [0.5, 0.4, 0.6]], dtype=np.float32)


def make_store(path, n_samples, seed=0, null=()):
    rng = np.random.default_rng(seed)
    root = zarr_store.open_group(path)
    samples = root.require_group("samples")
    keys = []
    for i in range(n_samples):
        key = f"{i:05d}_Dress_{i:06d}_0"
        keys.append(key)
        g = write_prediction_sample(samples, key, rng)
        if i in null:
            g.require_group("marching_cubes_mesh").array("volume_gradient_magnitude", np.full(1, np.nan, dtype=np.float32))
    return keys


# ------------------------------------------------------------------------------------------------ sampling and interpolation
def _doublearea_restated(v, f):
    v = v.astype(np.float64)
    out = []
    for t in f:
        r, s = v[t[0]] - v[t[2]], v[t[1]] - v[t[2]]
        acc = 0.0
        for x, y in ((0, 1), (1, 2), (2, 0)):
            p = r[x] * s[y] - r[y] * s[x]
            acc += p * p
        out.append(np.sqrt(acc))
    return np.array(out)


def test_mesh_sample_barycentric_restated():
    rng = np.random.default_rng(1)
    v, f = sheet(6, rng)
    bc, fi = M.mesh_sample_barycentric(v, f, 500, seed=3)
    w = _doublearea_restated(v, f)
    rs = np.random.RandomState(3)
    exp_fi = rs.choice(len(f), size=500, replace=True, p=w / w.sum())
    uv = rs.uniform(0, 1, size=(500, 2))
    for k in range(500):
        if uv[k, 0] + uv[k, 1] >= 1:
            uv[k] = 1 - uv[k]
    assert fi.dtype == f.dtype and np.array_equal(fi, exp_fi)
    assert bc.dtype == np.float64
    assert np.array_equal(bc[:, :2], uv) and np.array_equal(bc[:, 2], 1 - (uv[:, 0] + uv[:, 1]))
    # a fresh RandomState per call: two calls give the same draws
    bc2, fi2 = M.mesh_sample_barycentric(v, f, 500, seed=3)
    assert np.array_equal(bc, bc2) and np.array_equal(fi, fi2)
    assert np.array_equal(M.doublearea(v, f), w)


def _interp_restated(bc, verts, faces):
    out = np.zeros((len(bc), verts.shape[1]), dtype=verts.dtype)
    for n in range(len(bc)):
        for c in range(verts.shape[1]):
            acc = verts.dtype.type(0)
            for i in range(3):
                acc = verts.dtype.type(float(acc) + float(bc[n, i]) * float(verts[faces[n, i], c]))
            out[n, c] = acc
    return out


def test_barycentric_interpolation_rounds_every_partial_sum_to_the_vertex_dtype():
    rng = np.random.default_rng(2)
    verts = rng.random((40, 3)).astype(np.float32)
    faces = rng.integers(0, 40, (200, 3))
    bc = rng.random((200, 3))
    got = M.barycentric_interpolation(bc, verts, faces)
    assert got.dtype == np.float32 and np.array_equal(got, _interp_restated(bc, verts, faces))
    got64 = M.barycentric_interpolation(bc, verts.astype(np.float64), faces)
    assert got64.dtype == np.float64 and np.array_equal(got64, _interp_restated(bc, verts.astype(np.float64), faces))
    # a case where rounding each partial sum to float32 changes the result: 1 + 2^-24 rounds to 1 in float32, so the second term is lost;
    # accumulated in float64 and rounded once, (1 + 2^-24) + 2^-24 = 1 + 2^-23 is representable
    v = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], dtype=np.float32)
    one = M.barycentric_interpolation(np.array([[1.0, 1.0, 1.0]]), v, np.array([[0, 1, 2]]))
    assert one[0, 0] == np.float32(1.0)
    assert np.float32(1.0 + 2.0 ** -24 + 2.0 ** -24) == np.float32(1.0 + 2.0 ** -23) != one[0, 0]


def test_aabb_inverse_keeps_numpy_dtype_rules():
    data = np.random.default_rng(3).random((10, 3)).astype(np.float32)
    out = M.aabb_inverse(AABB, data)
    assert out.dtype == np.float32
    center = np.mean(AABB, axis=0)
    scale = 1 / np.max(AABB[1] - AABB[0])
    assert np.array_equal(out, (data - np.ones(3, np.float32) / 2) / scale + center)
    assert M.aabb_inverse(AABB.astype(np.float64), data).dtype == np.float64


# ------------------------------------------------------------------------------------------------ decision stump
def test_decision_stump_hand_cases():
    gm = np.array([0.1, 0.4, 0.2, 0.3], dtype=np.float32)
    # on surface exactly when gm >= 0.3: precision and recall both 1 at the third sorted value
    on = np.array([False, True, False, True])
    assert M.decision_stump_threshold(gm, on, 0.75) == np.float32(0.3)
    # tied gradient values: argsort's order decides, argmax takes the first maximal score
    gm_t = np.array([0.2, 0.2, 0.2, 0.5], dtype=np.float32)
    on_t = np.array([False, True, False, True])
    order = np.argsort(gm_t)
    s = on_t[order]
    tp = np.cumsum(s[::-1])[::-1]
    fp = np.cumsum(~s[::-1])[::-1]
    score = tp / (tp + fp) * 0.75 + tp / (tp + np.cumsum(s)) * 0.25
    assert M.decision_stump_threshold(gm_t, on_t, 0.75) == gm_t[order[np.argmax(score)]] == np.float32(0.5)
    # every neighbour on the surface: precision 1 everywhere, recall largest at the smallest value
    assert M.decision_stump_threshold(gm, np.ones(4, bool), 0.75) == np.float32(0.1)
    # no neighbour on the surface: recall 0 / 0 everywhere, no finite score -> min(gm)
    assert M.decision_stump_threshold(gm, np.zeros(4, bool), 0.75) == np.float32(0.1)
    gm2 = np.array([0.7, 0.6, 0.9], dtype=np.float32)
    assert M.decision_stump_threshold(gm2, np.zeros(3, bool), 0.5) == np.float32(0.6)


def test_threshold_metric_uses_the_nearest_ground_truth_vertex():
    sample = {"gt_marching_cubes_mesh/marching_cube_verts": np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32),
              "gt_marching_cubes_mesh/is_vertex_on_surface": np.array([False, True, True]),
              "marching_cubes_mesh/verts": np.array([[0.1, 0, 0], [1.9, 0, 0], [1.2, 0, 0], [-0.3, 0, 0]]),
              "marching_cubes_mesh/volume_gradient_magnitude": np.array([0.1, 0.8, 0.5, 0.2], np.float32)}
    r = M.optimal_gradient_threshold(sample, precision_weight=0.75, backend=CpuBackend())
    assert r == {"optimal_wnf_gradient_threshold": np.float32(0.5)}
    sample["gt_marching_cubes_mesh/marching_cube_verts"] = np.zeros((0, 3), np.float32)
    sample["gt_marching_cubes_mesh/is_vertex_on_surface"] = np.zeros(0, bool)
    with pytest.raises(IndexError):
        M.optimal_gradient_threshold(sample, backend=CpuBackend())


# ------------------------------------------------------------------------------------------------ pc and grip metrics
def test_pc_metrics_hand_example():
    aabb = np.array([[0, 0, 0], [2, 2, 2]], dtype=np.float64)        # inverse: x -> (x - 0.5) * 2 + 1 = 2 x
    gt = np.array([[0.5, 0.5, 0.5], [0.25, 0.5, 0.75]])
    pred = np.array([[0.5, 0.5, 1.0], [0.0, 0.5, 0.75]])
    r = M.pc_metrics({"point_cloud/gt_nocs": gt, "point_cloud/pred_nocs": pred}, aabb)
    assert list(r) == list(M.PC_COLUMNS)
    # in the inverse frame gt = [[1, 1, 1], [0.5, 1, 1.5]], pred = [[1, 1, 2], [0, 1, 1.5]]: diff = [[0, 0, 1], [-0.5, 0, 0]];
    # mirrored gt [[-1, 1, 1], [-0.5, 1, 1.5]]: pred - mirror = [[2, 0, 1], [0.5, 0, 0]]
    assert r["nocs_pc_error_distance"] == 0.75
    m = [np.sqrt(5.0), 0.5]
    assert r["nocs_pc_mirror_error_distance"] == np.mean(m)
    assert r["nocs_pc_min_agg_error_distance"] == np.mean([1.0, 0.5])
    assert r["nocs_pc_agg_min_error_distance"] == 0.75
    assert (r["nocs_pc_error_x"], r["nocs_pc_error_y"], r["nocs_pc_error_z"]) == (0.25, 0.0, 0.5)
    assert (r["nocs_pc_diff_std_x"], r["nocs_pc_diff_std_y"], r["nocs_pc_diff_std_z"]) == (0.25, 0.0, 0.5)


def test_grip_point_metrics_hand_example():
    aabb = np.array([[0, 0, 0], [1, 1, 1]], dtype=np.float64)        # inverse is the identity
    s = {"misc/gt_nocs_grip_point": np.array([-0.3, 0.0, 0.0]), "misc/pred_nocs_grip_point": np.array([0.3, 0.0, 0.4]),
         "misc/pred_global_nocs_grip_point": np.array([-0.3, 0.0, 0.1])}
    r = M.grip_point_metrics(s, aabb)
    assert list(r) == list(M.grip_point_columns())
    assert r["grip_point_error_distance_pc"] == np.linalg.norm([0.6, 0, 0.4])
    assert r["grip_point_mirror_error_distanc_pc"] == 0.4
    assert r["grip_point_min_error_distanc_pc"] == 0.4
    # (x - 0.5) / 1 + 0.5 is the identity up to rounding
    assert r["grip_point_error_distance_global"] == pytest.approx(0.1, rel=1e-14)
    assert r["grip_point_mirror_error_distanc_global"] == pytest.approx(np.hypot(0.6, 0.1), rel=1e-14)
    assert r["grip_point_min_error_distanc_global"] == r["grip_point_error_distance_global"]


# ------------------------------------------------------------------------------------------------ columns, overrides, nulls, errors
ALL = ("optimal_gradient_threshold", "pc", "grip_point", "chamfer", "hybrid_chamfer", "hausdorff")


@pytest.mark.parametrize("holes", [True, False])
def test_columns_per_function_in_order(tmp_path, holes):
    store = str(tmp_path / "prediction.zarr")
    make_store(store, 2)
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path / "out"), metrics=ALL, num_points=300, value_threshold=0.5,
                           predict_holes=holes, backend=CpuBackend())
    cham = (["chamfer_symmetrical_nocs", "chamfer_symmetrical_sim"] if holes else []) + \
        ["chamfer_symmetrical_nocs_no_hole", "chamfer_symmetrical_sim_no_hole", "chamfer_symmetrical_nocs_mc"]
    hyb = [f"hybrid_chamfer_{k}_{c}_{a}" for c in (["regular"] if holes else []) + ["no_hole"] for a in ("pred", "mirror", "min")
           for k in ("forward", "backward", "symmetrical")]
    haus = (["hausdorff_nocs", "hausdorff_sim"] if holes else []) + ["hausdorff_nocs_no_hole", "hausdorff_sim_no_hole", "hausdorff_nocs_mc"]
    grip = [f"grip_point_{m}_{k}" for k in ("pc", "global") for m in ("error_distance", "mirror_error_distanc", "min_error_distanc")]
    assert out["columns"] == ["optimal_wnf_gradient_threshold"] + list(M.PC_COLUMNS) + grip + cham + hyb + haus
    assert out["errors"] == []
    assert all(np.isfinite(out["table"][c]).all() for c in out["columns"])
    header = open(tmp_path / "out" / "all_metrics.csv").readline().rstrip("\n").split(",")
    assert header == [""] + out["columns"] + ["null_percentage"]


def test_one_search_call_per_sample_and_the_threshold_batch(tmp_path):
    store = str(tmp_path / "prediction.zarr")
    make_store(store, 3)
    be = CpuBackend()
    E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=ALL, num_points=200, backend=be)
    # one call for the three threshold searches, then one per sample: 5 x 2 chamfer + 2 x 2 x 2 hybrid pairs
    assert be.nn_calls == [3, 18, 18, 18]
    assert be.pm_calls == [10, 10, 10]


def test_override_rules(tmp_path):
    store = str(tmp_path / "prediction.zarr")
    keys = make_store(store, 3)
    be = CpuBackend()
    seen = []
    orig = M.plan_sampled_chamfer

    def spy(sample, nocs_aabb, **kw):
        seen.append(kw)
        return orig(sample, nocs_aabb, **kw)
    M.plan_sampled_chamfer = spy
    try:
        out = E.evaluate_store(store, AABB, output_dir=str(tmp_path), num_points=200, backend=be)
        thr = out["table"]["optimal_wnf_gradient_threshold"]
        agg = zarr_store.open_group(store, create=False)[E.DEFAULT_THRESHOLD_PATH]
        assert agg.shape == () and agg.dtype == np.float64 and agg == np.mean(thr)
        # the threshold of this run's aggregate, and the rest of the override set
        assert [k["value_threshold"] for k in seen] == [float(agg)] * len(keys)
        assert all(k["value_key"] == E.DEFAULT_VALUE_KEY and k["predict_holes"] is True and k["volume_task_space"] is False for k in seen)
        seen.clear()
        E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=("chamfer",), num_points=200, value_threshold=0.25, backend=be)
        assert [k["value_threshold"] for k in seen] == [0.25] * len(keys)
    finally:
        M.plan_sampled_chamfer = orig
    # threshold and pc take no override: a value_key that does not exist does not touch them
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=("optimal_gradient_threshold", "pc"), value_key="nope/none",
                           predict_holes=False, backend=be)
    assert out["errors"] == [] and np.isfinite(out["table"]["nocs_pc_error_distance"]).all()
    # a path that is not there: the error says so
    store2 = str(tmp_path / "fresh.zarr")
    make_store(store2, 1)
    with pytest.raises(KeyError, match="optimal_gradient_threshold"):
        E.evaluate_store(store2, AABB, output_dir=str(tmp_path), metrics=("chamfer",), backend=be)


def test_null_samples_and_null_percentage(tmp_path):
    store = str(tmp_path / "prediction.zarr")
    keys = make_store(store, 5, null=(1,))
    samples = zarr_store.open_group(store, create=False)["samples"]
    # empty array, missing array
    samples[keys[3]]["marching_cubes_mesh"].array("volume_gradient_magnitude", np.zeros(0, np.float32))
    import shutil
    shutil.rmtree(os.path.join(store, "samples", keys[4], "marching_cubes_mesh", "volume_gradient_magnitude"))
    assert [E.is_null(samples[k]) for k in keys] == [False, True, False, True, True]
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=("pc", "chamfer"), num_points=200, value_threshold=0.3,
                           backend=CpuBackend())
    for c in out["columns"]:
        v = out["table"][c]
        assert np.isnan(v[[1, 3, 4]]).all() and np.isfinite(v[[0, 2]]).all(), c
    summary = json.load(open(tmp_path / "summary.json"))
    assert summary["null_percentage"] == pytest.approx(0.6) and summary["null_percentage"] == float(np.float32(0.6))
    assert list(summary) == out["columns"] + ["null_percentage"]


def test_an_error_only_blanks_its_own_function_and_sample(tmp_path):
    store = str(tmp_path / "prediction.zarr")
    keys = make_store(store, 3)
    # sample 1: no triangle survives the hole threshold in hausdorff (np.argmax of no components), gt faces broken for the chamfers
    samples = zarr_store.open_group(store, create=False)["samples"]
    samples[keys[1]]["gt_mesh"].array("cloth_faces_tri", np.full((4, 3), 10 ** 6, dtype=np.int32))
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=ALL, num_points=200, value_threshold=0.3, backend=CpuBackend())
    failed = {(m, k) for m, k, _ in out["errors"]}
    assert failed == {("chamfer", keys[1]), ("hybrid_chamfer", keys[1]), ("hausdorff", keys[1])}
    for c in out["columns"]:
        v = out["table"][c]
        bad = c.startswith(("chamfer", "hybrid", "hausdorff"))
        assert np.isnan(v[1]) == bad, c
        assert np.isfinite(v[[0, 2]]).all(), c
    # an empty valid set: the chamfer column of that category is NaN, the hybrid function raises
    samples[keys[1]]["gt_mesh"].array("cloth_faces_tri", samples[keys[0]]["gt_mesh/cloth_faces_tri"])
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=("chamfer", "hybrid_chamfer"), num_points=200, value_threshold=2.0,
                           backend=CpuBackend())
    t = out["table"]
    assert np.isnan(t["chamfer_symmetrical_nocs"]).all() and np.isnan(t["chamfer_symmetrical_sim"]).all()
    assert np.isfinite(t["chamfer_symmetrical_nocs_no_hole"]).all()
    assert all(np.isnan(t[c]).all() for c in M.hybrid_chamfer_columns(True))
    assert {m for m, _, _ in out["errors"]} == {"hybrid_chamfer"}


# ------------------------------------------------------------------------------------------------ outputs
def test_describe_nanmean_and_summary(tmp_path):
    v = np.array([1.0, np.nan, 3.0, 4.0, 10.0])
    d = E.describe(v)
    w = v[~np.isnan(v)]
    assert d == [4.0, np.mean(w), np.std(w, ddof=1), 1.0, 2.5, 3.5, 5.5, 10.0]
    assert np.isnan(E.describe([np.nan, 1.0])[2]) and E.describe([np.nan])[0] == 0.0
    cols = ["a", "b"]
    table = {"a": v, "b": np.full(5, np.nan)}
    null = np.array([False, True, False, False, False])
    summ = E.write_outputs(str(tmp_path), cols, table, null)
    assert summ["a"] == 4.5 and np.isnan(summ["b"]) and summ["null_percentage"] == float(np.float32(0.2))   # a float32 mean, as pandas'
    rows = open(tmp_path / "all_metrics.csv").read().splitlines()
    assert rows[0] == ",a,b,null_percentage" and rows[1] == "0,1.0,,0.0" and rows[2] == "1,,,1.0"
    agg = open(tmp_path / "all_metrics_agg.csv").read().splitlines()
    assert [r.split(",")[0] for r in agg] == ["", "count", "mean", "std", "min", "25%", "50%", "75%", "max"]
    assert agg[1] == "count,4.0,0.0,5.0"
    js = json.load(open(tmp_path / "summary.json"))
    assert list(js) == ["a", "b", "null_percentage"] and js["a"] == 4.5


def test_per_sample_arrays_in_the_store(tmp_path):
    store = str(tmp_path / "prediction.zarr")
    keys = make_store(store, 3, null=(2,))
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=("optimal_gradient_threshold", "pc"), backend=CpuBackend())
    root = zarr_store.open_group(store, create=False)
    assert list(root["summary/metrics/per_sample/sample_keys"]) == keys
    for c in out["columns"]:
        got = root[f"summary/metrics/per_sample/{c}"]
        assert got.dtype == np.float64 and np.array_equal(got, out["table"][c], equal_nan=True)
        assert root[f"summary/metrics/aggregate/{c}"] == np.nanmean(out["table"][c])


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_defaults_follow_eval_default_yaml():
    a = E.build_parser().parse_args(["--prediction", "p.zarr", "--zarr_in", "d.zarr"])
    assert a.metrics == ["optimal_gradient_threshold", "pc", "chamfer", "hybrid_chamfer"]
    assert a.precision_weight == 0.75 and a.num_points == 10000 and a.seed == 0
    assert a.value_threshold == "summary/metrics/aggregate/optimal_wnf_gradient_threshold"
    assert a.value_key == "marching_cubes_mesh/volume_gradient_magnitude"
    assert a.predict_holes is True and a.volume_task_space is False and a.output_dir == "."
    b = E.build_parser().parse_args(["--prediction", "p", "--nocs_aabb", "0", "0", "0", "1", "1", "1", "--value_threshold", "0.2",
                                     "--no_predict_holes", "--metrics", "grip_point", "hausdorff"])
    assert b.value_threshold == 0.2 and b.predict_holes is False and b.metrics == ["grip_point", "hausdorff"]


def test_cli_refuses_geodesic(tmp_path, capsys):
    with pytest.raises(SystemExit):
        E.main(["--prediction", str(tmp_path), "--nocs_aabb", "0", "0", "0", "1", "1", "1", "--metrics", "geodesic"], backend=CpuBackend())
    assert "not implemented" in capsys.readouterr().err
    with pytest.raises(ValueError, match="not implemented"):
        E.evaluate_store(str(tmp_path), AABB, metrics=("geodesic",), backend=CpuBackend())


def test_cli_end_to_end_on_the_cpu_backend(tmp_path):
    store, ds = str(tmp_path / "prediction.zarr"), str(tmp_path / "dataset.zarr")
    make_store(store, 2)
    zarr_store.open_group(ds).require_group("summary").array("cloth_canonical_aabb_union", AABB)
    out = E.main(["--prediction", store, "--zarr_in", ds, "--output_dir", str(tmp_path / "o"), "--num_points", "300"], backend=CpuBackend())
    assert out["errors"] == [] and len(out["columns"]) == 1 + 10 + 5 + 18
    for f in ("all_metrics.csv", "all_metrics_agg.csv", "summary.json"):
        assert os.path.exists(tmp_path / "o" / f)


# ================================================================================================================================
# An independent restatement of eval.py's metric functions (eval.py:58-580), written from its semantics with numpy, scipy's cKDTree,
# the Ericson brute force above and scipy's connected components; it does not use garmentnets_amd.common.metrics.
def zarr_read(store, path):
    """minimal Zarr v2 reader (spec only: .zarray, C order, zlib or no compressor)"""
    import itertools
    import zlib
    base = os.path.join(store, path)
    meta = json.load(open(os.path.join(base, ".zarray")))
    assert meta["zarr_format"] == 2 and meta["order"] == "C" and not meta.get("filters")
    shape, chunks, dt = meta["shape"], meta["chunks"], np.dtype(meta["dtype"])
    out = np.zeros(shape, dtype=dt)
    for idx in itertools.product(*[range(-(-s // c)) for s, c in zip(shape, chunks)]):
        f = os.path.join(base, ".".join(map(str, idx)) if idx else "0")
        if not os.path.exists(f):
            continue
        raw = open(f, "rb").read()
        if meta["compressor"] is not None:
            assert meta["compressor"]["id"] == "zlib"
            raw = zlib.decompress(raw)
        block = np.frombuffer(raw, dtype=dt).reshape(chunks)
        sel = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, shape))
        out[sel] = block[tuple(slice(0, s.stop - s.start) for s in sel)]
    return out


def _r_inverse(aabb, x):                        # AABBNormalizer(aabb).inverse(x)
    center = np.mean(aabb, axis=0)
    scale = 1 / np.max(aabb[1] - aabb[0])
    return (x - np.ones((3,), dtype=aabb.dtype) / 2) / scale + center


def _r_sample(verts, faces, n, seed):           # mesh_sample_barycentric with igl.doublearea
    w = _doublearea_restated(verts, faces)
    w = w / np.sum(w)
    rs = np.random.RandomState(seed=seed)
    fi = rs.choice(len(faces), size=n, replace=True, p=w).astype(faces.dtype)
    uv = rs.uniform(0, 1, size=(n, 2))
    flip = np.sum(uv, axis=1) >= 1
    uv[flip] = 1 - uv[flip]
    bc = np.zeros((n, 3), dtype=uv.dtype)
    bc[:, :2] = uv
    bc[:, 2] = 1 - np.sum(uv, axis=1)
    return bc, fi


def _r_interp(bc, verts, faces):                # barycentric_interpolation, one column at a time
    out = np.zeros((len(bc), verts.shape[1]), dtype=verts.dtype)
    for c in range(verts.shape[1]):
        for i in range(bc.shape[1]):
            out[:, c] += bc[:, i] * verts[:, c][faces[:, i]]
    return out


def _r_delete_invalid(verts, faces, keep):      # common/marching_cubes_util.py:38-52
    ok = keep[faces[:, 0]] & keep[faces[:, 1]] & keep[faces[:, 2]]
    f = faces[ok]
    used = np.unique(f.flatten())
    remap = np.zeros(len(verts), dtype=faces.dtype)
    remap[used] = np.arange(len(used))
    return verts[used], remap[f]


def _r_largest_cc(faces):                       # igl.adjacency_matrix + igl.connected_components + argmax
    n = int(faces.max()) + 1 if len(faces) else 0
    i = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2], faces[:, 1], faces[:, 2], faces[:, 0]])
    j = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0], faces[:, 0], faces[:, 1], faces[:, 2]])
    _, lab = connected_components(coo_matrix((np.ones(len(i)), (i, j)), shape=(n, n)), directed=True, connection="weak")
    sizes = np.bincount(lab, minlength=0)
    return lab == np.argmax(sizes)


def _r_sqdist_to_mesh(p, v, f):
    v = v.astype(np.float64)
    p = p.astype(np.float64)
    return np.concatenate([closest_point_sqdist(p[k:k + 64], v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]).min(1) for k in range(0, len(p), 64)])


def r_threshold(rd, precision_weight):
    gt_v, on = rd("gt_marching_cubes_mesh/marching_cube_verts"), rd("gt_marching_cubes_mesh/is_vertex_on_surface")
    pv, gm = rd("marching_cubes_mesh/verts"), rd("marching_cubes_mesh/volume_gradient_magnitude")
    _, idx = cKDTree(gt_v).query(pv, k=1)
    nn_on = on[idx]
    order = np.argsort(gm)
    s = nn_on[order]
    fn, tp, fp = np.cumsum(s), np.cumsum(s[::-1])[::-1], np.cumsum(~s[::-1])[::-1]
    precision, recall = tp / (tp + fp), tp / (tp + fn)
    score = precision * precision_weight + recall * (1 - precision_weight)
    thr = gm[order[np.argmax(score)]] if np.any(np.isfinite(score)) else gm.min()
    return {"optimal_wnf_gradient_threshold": thr}


def r_pc(rd, aabb):
    gt, pred = _r_inverse(aabb, rd("point_cloud/gt_nocs")), _r_inverse(aabb, rd("point_cloud/pred_nocs"))
    diff = pred - gt
    mg = gt.copy()
    mg[:, 0] = -mg[:, 0]
    e, me = np.linalg.norm(diff, axis=1), np.linalg.norm(pred - mg, axis=1)
    out = {"nocs_pc_error_distance": np.mean(e), "nocs_pc_mirror_error_distance": np.mean(me),
           "nocs_pc_min_agg_error_distance": np.mean(np.minimum(e, me)), "nocs_pc_agg_min_error_distance": np.minimum(np.mean(e), np.mean(me))}
    std, err = np.std(diff, axis=0), np.mean(np.abs(diff), axis=0)
    out.update({f"nocs_pc_diff_std_{a}": std[i] for i, a in enumerate("xyz")})
    out.update({f"nocs_pc_error_{a}": err[i] for i, a in enumerate("xyz")})
    return out


def r_grip(rd, aabb):
    gt = _r_inverse(aabb, rd("misc/gt_nocs_grip_point"))
    out = {}
    for key, path in (("pc", "misc/pred_nocs_grip_point"), ("global", "misc/pred_global_nocs_grip_point")):
        p = _r_inverse(aabb, rd(path))
        m = p.copy()
        m[0] = -m[0]
        e, me = np.linalg.norm(p - gt), np.linalg.norm(m - gt)
        out.update({f"grip_point_error_distance_{key}": e, f"grip_point_mirror_error_distanc_{key}": me, f"grip_point_min_error_distanc_{key}": min(e, me)})
    return out


def _r_inputs(rd, aabb, task_space=False):
    pv, pf, psim = rd("marching_cubes_mesh/verts"), rd("marching_cubes_mesh/faces"), rd("marching_cubes_mesh/warp_field")
    if task_space:
        pv, psim = psim, pv
    gf, gn, gs = rd("gt_mesh/cloth_faces_tri"), rd("gt_mesh/cloth_nocs_verts"), rd("gt_mesh/cloth_verts")
    return _r_inverse(aabb, pv), pf, psim, gf, _r_inverse(aabb, gn), gs


def _r_samples(rd, aabb, n, seed, thr, value_key):
    pv, pf, psim, gf, gn, gs = _r_inputs(rd, aabb)
    pbc, pfi = _r_sample(pv, pf, n, seed)
    p_n, p_s = _r_interp(pbc, pv, pf[pfi]), _r_interp(pbc, psim, pf[pfi])
    gbc, gfi = _r_sample(gn, gf, n, seed)
    g_n, g_s = _r_interp(gbc, gn, gf[gfi]), _r_interp(gbc, gs, gf[gfi])
    valid = np.squeeze(_r_interp(pbc, np.expand_dims(rd(value_key), axis=1), pf[pfi])) > thr
    return p_n, p_s, g_n, g_s, valid


def r_chamfer(rd, aabb, n, seed, thr, value_key, holes):
    p_n, p_s, g_n, g_s, valid = _r_samples(rd, aabb, n, seed, thr, value_key)
    mv, mf, on = (rd("gt_marching_cubes_mesh/" + k) for k in ("marching_cube_verts", "marching_cube_faces", "is_vertex_on_surface"))
    sv, sf = _r_delete_invalid(_r_inverse(aabb, mv), mf, on)
    mbc, mfi = _r_sample(sv, sf, n, seed)
    g_mc = _r_interp(mbc, sv, sf[mfi])

    def ch(p, g):
        fd, _ = cKDTree(g).query(p, k=1)
        bd, _ = cKDTree(p).query(g, k=1)
        return np.mean([np.mean(fd), np.mean(bd)])
    out = {}
    if holes:
        out["chamfer_symmetrical_nocs"] = ch(p_n[valid], g_n)
        out["chamfer_symmetrical_sim"] = ch(p_s[valid], g_s)
    out["chamfer_symmetrical_nocs_no_hole"] = ch(p_n, g_n)
    out["chamfer_symmetrical_sim_no_hole"] = ch(p_s, g_s)
    out["chamfer_symmetrical_nocs_mc"] = ch(g_mc, g_n)
    return out


def r_hybrid(rd, aabb, n, seed, thr, value_key, holes):
    p_n, p_s, g_n, g_s, valid = _r_samples(rd, aabb, n, seed, thr, value_key)

    def hy(pn, ps):
        _, fi = cKDTree(g_n).query(pn, k=1)
        _, bi = cKDTree(pn).query(g_n, k=1)
        f = np.mean(np.linalg.norm(ps - g_s[fi], axis=1))
        b = np.mean(np.linalg.norm(g_s - ps[bi], axis=1))
        return {"forward": f, "backward": b, "symmetrical": np.mean([f, b])}
    out = {}
    for cat, pn, ps in ([("regular", p_n[valid], p_s[valid])] if holes else []) + [("no_hole", p_n, p_s)]:
        mpn = pn.copy()
        mpn[:, 0] = -mpn[:, 0]
        res = {"pred": hy(pn, ps), "mirror": hy(mpn, ps)}
        res["min"] = {k: min(res["pred"][k], res["mirror"][k]) for k in res["pred"]}
        for aug in ("pred", "mirror", "min"):
            for k in ("forward", "backward", "symmetrical"):
                out[f"hybrid_chamfer_{k}_{cat}_{aug}"] = res[aug][k]
    return out


def r_hausdorff(rd, aabb, thr, value_key, holes):
    pv, pf, psim, gf, gn, gs = _r_inputs(rd, aabb)
    mv, mf, on = (rd("gt_marching_cubes_mesh/" + k) for k in ("marching_cube_verts", "marching_cube_faces", "is_vertex_on_surface"))
    sv, sf = _r_delete_invalid(_r_inverse(aabb, mv), mf, on)
    cc = _r_largest_cc(sf)
    cv, cf = _r_delete_invalid(sv, sf, cc)

    def hd(va, fa, vb, fb):
        return np.sqrt(max(_r_sqdist_to_mesh(vb, va, fa).max(), _r_sqdist_to_mesh(va, vb, fb).max()))
    out = {}
    if holes:
        keep = rd(value_key) > thr
        hv, hf = _r_delete_invalid(pv, pf, keep)
        hs, _ = _r_delete_invalid(psim, pf, keep)
        cc = _r_largest_cc(hf)
        hv2, hf2 = _r_delete_invalid(hv, hf, cc)
        hs2, _ = _r_delete_invalid(hs, hf, cc)
        out["hausdorff_nocs"] = hd(gn, gf, hv2, hf2)
        out["hausdorff_sim"] = hd(gs, gf, hs2, hf2)
    out["hausdorff_nocs_no_hole"] = hd(gn, gf, pv, pf)
    out["hausdorff_sim_no_hole"] = hd(gs, gf, psim, pf)
    out["hausdorff_nocs_mc"] = hd(gn, gf, cv, cf)
    return out


def r_evaluate(store, aabb, metrics, num_points=10000, seed=0, precision_weight=0.75, value_threshold=None,
               value_key="marching_cubes_mesh/volume_gradient_magnitude", holes=True):
    """eval.py's main loop over the store: {column: float64 per sample}; a failing (function, sample) gives NaN in that function's columns"""
    keys = sorted(k for k in os.listdir(os.path.join(store, "samples")) if not k.startswith("."))

    def reader(k):
        return lambda path: zarr_read(store, os.path.join("samples", k, path))

    def null(k):
        p = os.path.join(store, "samples", k, "marching_cubes_mesh", "volume_gradient_magnitude")
        if not os.path.exists(os.path.join(p, ".zarray")):
            return True
        a = zarr_read(store, os.path.join("samples", k, "marching_cubes_mesh", "volume_gradient_magnitude"))
        return len(a) == 0 or np.isnan(a.flatten()[0])
    live = [i for i, k in enumerate(keys) if not null(k)]
    table = {}

    def run(fn):
        for i in live:
            try:
                with np.errstate(all="ignore"):
                    r = fn(reader(keys[i]))
            except Exception:            # noqa: BLE001
                continue
            for c, v in r.items():
                table.setdefault(c, np.full(len(keys), np.nan))[i] = float(v)
    if "optimal_gradient_threshold" in metrics:
        run(lambda rd: r_threshold(rd, precision_weight))
    thr = value_threshold if value_threshold is not None else np.nanmean(table["optimal_wnf_gradient_threshold"])
    if "pc" in metrics:
        run(lambda rd: r_pc(rd, aabb))
    if "grip_point" in metrics:
        run(lambda rd: r_grip(rd, aabb))
    if "chamfer" in metrics:
        run(lambda rd: r_chamfer(rd, aabb, num_points, seed, thr, value_key, holes))
    if "hybrid_chamfer" in metrics:
        run(lambda rd: r_hybrid(rd, aabb, num_points, seed, thr, value_key, holes))
    if "hausdorff" in metrics:
        run(lambda rd: r_hausdorff(rd, aabb, thr, value_key, holes))
    return table


EXACT_PREFIXES = ("optimal_wnf", "nocs_pc", "grip_point")


def assert_matches_restatement(out, ref, rtol=1e-12):
    """every per-sample value of evaluate_store's `out` against r_evaluate's `ref`: threshold, pc and grip bit-equal, the rest within rtol"""
    for c in out["columns"]:
        g = out["table"][c]
        r = ref.get(c, np.full(len(g), np.nan))
        assert np.array_equal(np.isnan(g), np.isnan(r)), (c, g, r)
        ok = ~np.isnan(r)
        if c.startswith(EXACT_PREFIXES):
            assert np.array_equal(g[ok], r[ok]), (c, g, r)
        else:
            assert np.all(np.abs(g[ok] - r[ok]) <= rtol * np.abs(r[ok])), (c, g, r)
    assert set(ref) <= set(out["columns"])


@pytest.mark.parametrize("holes", [True, False])
def test_every_value_against_the_restatement_of_eval_py(tmp_path, holes):
    store = str(tmp_path / "prediction.zarr")
    make_store(store, 4, seed=7, null=(2,))
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=ALL, num_points=500, predict_holes=holes, backend=CpuBackend())
    ref = r_evaluate(store, AABB, ALL, num_points=500, holes=holes)
    assert out["errors"] == []
    assert_matches_restatement(out, ref)
    # a fixed threshold high enough that the hole categories change, and an empty valid set in one sample's chamfer
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=("chamfer", "hybrid_chamfer", "hausdorff"), num_points=500,
                           value_threshold=0.35, predict_holes=holes, backend=CpuBackend())
    assert_matches_restatement(out, r_evaluate(store, AABB, ("chamfer", "hybrid_chamfer", "hausdorff"), num_points=500, value_threshold=0.35,
                                               holes=holes))


def test_restatement_tells_the_metrics_apart(tmp_path):
    """the restatement is sensitive to what it checks: forward / backward swapped, or distances taken in NOCS space, differ"""
    store = str(tmp_path / "prediction.zarr")
    make_store(store, 1, seed=3)
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=("hybrid_chamfer", "hausdorff"), num_points=400, value_threshold=0.2,
                           backend=CpuBackend())
    t = out["table"]
    assert t["hybrid_chamfer_forward_no_hole_pred"][0] != t["hybrid_chamfer_backward_no_hole_pred"][0]
    assert t["hausdorff_nocs_no_hole"][0] != t["hausdorff_sim_no_hole"][0] != t["hausdorff_nocs_mc"][0]


def test_one_failing_sample_does_not_blank_the_batched_threshold(tmp_path):
    store = str(tmp_path / "prediction.zarr")
    keys = make_store(store, 3)
    samples = zarr_store.open_group(store, create=False)["samples"]
    samples[keys[1]]["marching_cubes_mesh"].array("verts", np.zeros((81, 2)))          # not (N, 3): the device wrapper raises
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=("optimal_gradient_threshold",), backend=CpuBackend())
    t = out["table"]["optimal_wnf_gradient_threshold"]
    assert np.isnan(t[1]) and np.isfinite(t[[0, 2]]).all()
    assert [(m, k) for m, k, _ in out["errors"]] == [("optimal_gradient_threshold", keys[1])]


def test_grip_point_dereferences_the_threshold_path_as_eval_py_does(tmp_path):
    store = str(tmp_path / "prediction.zarr")
    make_store(store, 1)
    with pytest.raises(KeyError, match="optimal_gradient_threshold"):
        E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=("grip_point",), backend=CpuBackend())
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path), metrics=("grip_point",), value_threshold=0.3, backend=CpuBackend())
    assert out["errors"] == []
