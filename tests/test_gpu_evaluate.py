"""GPU (-m gpu): the fp64 evaluation distances of csrc/eval_dist.hip (ops.nearest_neighbor_f64*, ops.point_mesh_sqdist*) against
independent numpy / scipy restatements, and `python -m garmentnets_amd.evaluate` end to end on a store written by predict.main."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu

from garmentnets_amd import evaluate as E, ops, synthetic as S  # noqa: E402
from garmentnets_amd.common import metrics as M  # noqa: E402
from garmentnets_amd.io import zarr_store  # noqa: E402
from test_evaluate_host import CpuBackend, assert_matches_restatement, closest_point_sqdist, r_evaluate, sheet  # noqa: E402

DEV = "cuda:0"


def _d(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device=DEV)


def _pm(q, v, f):
    i, d2 = ops.point_mesh_sqdist(_d(q), _d(v), _d(f, torch.int32))
    return i.cpu().numpy(), d2.cpu().numpy()


# ------------------------------------------------------------------------------------------------ point -> mesh
def test_point_mesh_analytic_cases():
    tri_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float64)
    tri_f = np.array([[0, 1, 2]])
    h = 0.375
    q = np.array([[0.25, 0.25, h],          # above the interior
                  [0.5, -0.5, 0.0],         # beyond edge v0 v1 (in the plane)
                  [-0.5, 0.5, 0.25],        # beyond edge v0 v2
                  [1.0, 1.0, 0.0],          # beyond edge v1 v2
                  [-1.0, -1.0, 0.0],        # beyond vertex v0
                  [2.0, -0.5, 0.0],         # beyond vertex v1
                  [-0.5, 2.0, 0.5],         # beyond vertex v2
                  [0.1, 0.2, 0.0]])         # in the plane, inside
    exp = np.array([h * h, 0.25, 0.25 + 0.0625, 0.5, 2.0, 1.25, 0.5 ** 2 + 1.0 + 0.25, 0.0])
    i, d2 = _pm(q, tri_v, tri_f)
    assert np.array_equal(i, np.zeros(len(q))) and np.allclose(d2, exp, rtol=1e-15, atol=0)
    # degenerate triangles: zero area (collinear), a repeated vertex, all three vertices equal -> distances to their edges / point
    dv = np.array([[0, 0, 0], [1, 1, 1], [3, 3, 3], [5, 0, 0], [5, 2, 0], [9, 9, 9]], dtype=np.float64)
    for face, p, e in (([0, 1, 2], [3, 3, 0], 6.0),        # the foot of (3,3,0) on the line x=y=z is (2,2,2): 1 + 1 + 4
                       ([3, 3, 4], [6, 1, 0], 1.0),
                       ([5, 5, 5], [9, 9, 10], 1.0)):
        i, d2 = _pm([p], dv, [face])
        ref = closest_point_sqdist(np.array([p], np.float64), dv[[face[0]]], dv[[face[1]]], dv[[face[2]]])[0, 0]
        assert i[0] == 0 and d2[0] == ref == e, (face, d2, ref)
    # almost collinear triangles with non-integer coordinates (det = a c - b^2 is rounding noise): the distance is that to the edges
    from test_evaluate_host import _seg_sqdist
    rng = np.random.default_rng(9)
    u = np.array([0.3, 0.5, 0.7])
    a0 = np.array([0.1, 0.2, 0.3])
    sv = np.stack([a0, a0 + 0.7 * u, a0 + 1.3 * u])
    sq = a0 + rng.uniform(-0.5, 2.0, (200, 1)) * u + 0.05 * rng.standard_normal((200, 3))
    i, d2 = _pm(sq, sv, [[0, 1, 2]])
    p = sq[:, None, :]
    A, B, C = sv[[0]], sv[[1]], sv[[2]]
    seg = np.minimum(np.minimum(_seg_sqdist(p, A, B), _seg_sqdist(p, A, C)), _seg_sqdist(p, B, C))[:, 0]
    assert np.all(np.abs(d2 - seg) <= 1e-12 * np.maximum(seg, 1.0))
    # a closed cube [0,1]^3 (12 triangles): inside, outside a face, outside an edge, outside a corner
    cv = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)
    cf = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]])
    cq = np.array([[0.5, 0.5, 0.25], [0.5, 0.5, 1.5], [1.5, 1.5, 0.5], [2.0, 2.0, 2.0], [0.5, 0.1, 0.5]])
    _, d2 = _pm(cq, cv, cf)
    assert np.allclose(d2, [0.0625, 0.25, 0.5, 3.0, 0.01], rtol=1e-15, atol=0)
    # NaN query, empty mesh
    i, d2 = _pm([[np.nan, 0, 0], [0.2, 0.2, 1.0]], tri_v, tri_f)
    assert np.isnan(d2[0]) and d2[1] == 1.0
    i, d2 = _pm([[0.0, 0.0, 0.0]], tri_v, np.zeros((0, 3), np.int64))
    assert i[0] == -1 and d2[0] == np.inf


def test_point_mesh_random_meshes_many_tiles():
    rng = np.random.default_rng(0)
    v = rng.random((20000, 3))
    f = rng.integers(0, len(v), (40000, 3))
    q = rng.random((20000, 3)) * 1.2 - 0.1
    i, d2 = _pm(q, v, f)
    diag2 = 3.0
    # 400 random queries, and every query of three 256-query blocks: the first, one in the middle and the last, partial one (32 queries)
    blocks = np.concatenate([np.arange(0, 256), np.arange(40 * 256, 41 * 256), np.arange(78 * 256, len(q))])
    sel = np.unique(np.concatenate([rng.choice(len(q), 400, replace=False), blocks]))
    ref = np.concatenate([closest_point_sqdist(q[sel[k:k + 25]], v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]) for k in range(0, len(sel), 25)])
    best = np.min(ref, axis=1)
    tol = 1e-12 * np.maximum(best, diag2)
    assert np.all(np.abs(d2[sel] - best) <= tol)
    second = np.partition(ref, 1, axis=1)[:, 1]
    clear = (second - best) > tol
    assert clear.mean() > 0.5          # a dense soup of 40 000 random triangles: many queries sit within the tolerance of two
    assert np.array_equal(i[sel][clear], np.argmin(ref, axis=1)[clear])


def test_point_mesh_ragged_pairs_and_bad_faces():
    rng = np.random.default_rng(1)
    meshes, queries = [], []
    for nq, nv, nf in ((300, 50, 129), (0, 10, 7), (77, 0, 0), (513, 200, 1), (1, 30, 300)):
        v = rng.random((nv, 3))
        f = rng.integers(0, max(nv, 1), (nf, 3))
        meshes.append((v, f))
        queries.append(rng.random((nq, 3)))
    res = ops.point_mesh_sqdist_batch([_d(q) for q in queries], [(_d(v), _d(f, torch.int64)) for v, f in meshes])
    for q, (v, f), (i, d2) in zip(queries, meshes, res):
        i, d2 = i.cpu().numpy(), d2.cpu().numpy()
        assert len(i) == len(q)
        if len(f) == 0:
            assert (i == -1).all() and np.isinf(d2).all()
            continue
        if len(q):
            ref = closest_point_sqdist(q, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
            assert np.allclose(d2, ref.min(1), rtol=1e-12, atol=1e-15)
    with pytest.raises(IndexError):
        ops.point_mesh_sqdist(_d(rng.random((5, 3))), _d(rng.random((4, 3))), _d([[0, 1, 4]], torch.int32))
    # a pair without queries still has its faces checked
    with pytest.raises(IndexError):
        ops.point_mesh_sqdist_batch([_d(np.zeros((0, 3))), _d(rng.random((3, 3)))],
                                    [(_d(rng.random((4, 3))), _d([[0, 1, -1]], torch.int32)), (_d(rng.random((4, 3))), _d([[0, 1, 2]], torch.int32))])


# ------------------------------------------------------------------------------------------------ nearest neighbour
def test_nearest_neighbor_f64_against_ckdtree():
    rng = np.random.default_rng(2)
    r = rng.random((7000, 3))
    q = rng.random((5000, 3))
    i, d2 = [t.cpu().numpy() for t in ops.nearest_neighbor_f64(_d(q), _d(r))]
    d, j = cKDTree(r).query(q, k=1)
    assert np.array_equal(i, j)
    assert np.all(np.abs(np.sqrt(d2) - d) <= np.spacing(d))
    # exact ties go to the lowest index; ragged pairs with empty sets
    rt = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [1.0, 0, 0]])
    res = ops.nearest_neighbor_f64_batch([_d([[0.0, 0, 0], [2.0, 0, 0]]), _d(np.zeros((0, 3))), _d(q[:300]), _d([[0.0, 0, 0]])],
                                         [_d(rt), _d(r), _d(r[:257]), _d(np.zeros((0, 3)))])
    assert res[0][0].cpu().tolist() == [0, 0]
    assert len(res[1][0]) == 0
    assert np.array_equal(res[2][0].cpu().numpy(), cKDTree(r[:257]).query(q[:300], k=1)[1])
    assert res[3][0].cpu().tolist() == [-1] and res[3][1].cpu().tolist() == [np.inf]
    # one query tensor against two reference sets: two sets of output rows
    qq = _d(q[:100])
    (i1, _), (i2, _) = ops.nearest_neighbor_f64_batch([qq, qq], [_d(r[:50]), _d(r[50:120])])
    assert np.array_equal(i1.cpu().numpy(), cKDTree(r[:50]).query(q[:100], k=1)[1])
    assert np.array_equal(i2.cpu().numpy(), cKDTree(r[50:120]).query(q[:100], k=1)[1])


# ------------------------------------------------------------------------------------------------ end to end
def _zarr_read(store, path):
    """independent minimal Zarr v2 reader (spec only: .zarray, C order, zlib or no compressor)"""
    import itertools
    import zlib
    base = os.path.join(store, path)
    meta = json.load(open(os.path.join(base, ".zarray")))
    assert meta["zarr_format"] == 2 and meta["order"] == "C" and not meta.get("filters")
    shape, chunks, dt = meta["shape"], meta["chunks"], np.dtype(meta["dtype"])
    out = np.zeros(shape, dtype=dt)
    for idx in itertools.product(*[range(-(-s // c)) for s, c in zip(shape, chunks)]):
        raw = open(os.path.join(base, ".".join(map(str, idx)) if idx else "0"), "rb").read()
        if meta["compressor"] is not None:
            assert meta["compressor"]["id"] == "zlib"
            raw = zlib.decompress(raw)
        block = np.frombuffer(raw, dtype=dt).reshape(chunks)
        sel = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, shape))
        out[sel] = block[tuple(slice(0, s.stop - s.start) for s in sel)]
    return out


def write_dataset(path, n_samples, seed=0, n_gt=14, n_mc=12):
    """a garmentnets dataset store whose gt_mesh / marching_cube_mesh are triangulated surfaces (height-field sheets) + the summary AABBs"""
    rng = np.random.default_rng(seed)
    root = zarr_store.open_group(path)
    summ = root.require_group("summary")
    summ.array("cloth_aabb_union", np.array([[-0.4, -0.4, -0.9], [0.4, 0.4, 0.05]], dtype=np.float32))
    summ.array("cloth_canonical_aabb_union", np.array([[-0.45, -0.2, -0.5], [0.45, 0.3, 0.4]], dtype=np.float32))
    for i in range(n_samples):
        sg = root.require_group("samples").require_group(f"{i:05d}_Dress_{i:06d}_0")
        sg.put_attrs({"scale": 1.0, "gender": 0, "sample_id": f"{i:05d}_Dress", "garment_name": "Dress", "grip_vertex_idx": 3})
        x, pos, _ = S.synthetic_cloud(1, 2400, seed=90 + i)
        pos = pos.numpy()
        nocs = ((pos - pos.min(0)) / (pos.max(0) - pos.min(0))).astype(np.float32)
        pc, mesh, mc = sg.require_group("point_cloud"), sg.require_group("mesh"), sg.require_group("marching_cube_mesh")
        pc.array("point", pos)
        pc.array("nocs", nocs)
        pc.array("rgb", (x.numpy() * 255).astype(np.uint8))
        pc.array("sizes", np.array([600, 600, 600, 600], dtype=np.int64))
        gv, gf = sheet(n_gt, rng)
        mesh.array("cloth_verts", gv * 0.6 - 0.3)
        mesh.array("cloth_nocs_verts", gv)
        mesh.array("cloth_faces_tri", gf)
        mv, mf = sheet(n_mc, rng, z=0.01)
        mc.array("marching_cube_verts", mv)
        mc.array("marching_cube_faces", mf)
        on = np.ones(len(mv), dtype=bool)
        on[rng.choice(len(mv), 6, replace=False)] = False
        mc.array("is_vertex_on_surface", on)


ALL = ("optimal_gradient_threshold", "pc", "grip_point", "chamfer", "hybrid_chamfer", "hausdorff")


def test_evaluate_end_to_end(tmp_path):
    from garmentnets_amd import predict as PR
    din, dout = str(tmp_path / "dataset.zarr"), str(tmp_path / "prediction.zarr")
    write_dataset(din, 3)
    PR.main(["--zarr_in", din, "--zarr_out", dout, "--num_pc_sample", "1800", "--num_views", "3", "--grid", "16", "--volume_size", "24",
             "--auto_level", "--static_epoch_seed", "--subset", "all"])
    keys = sorted(os.listdir(os.path.join(dout, "samples")))
    keys = [k for k in keys if not k.startswith(".")]
    # one sample forced to predict's NaN placeholder
    zarr_store.open_group(dout, create=False)["samples"][keys[1]]["marching_cubes_mesh"].array(
        "volume_gradient_magnitude", np.full(1, np.nan, dtype=np.float32))
    args = ["--prediction", dout, "--zarr_in", din, "--metrics", *ALL, "--num_points", "3000"]
    gpu = E.main(args + ["--output_dir", str(tmp_path / "a")])
    assert gpu["errors"] == []
    files = {f: open(tmp_path / "a" / f).read() for f in ("all_metrics.csv", "all_metrics_agg.csv", "summary.json")}
    # every per-sample value against the test's restatement of eval.py's functions (cKDTree, Ericson brute force, scipy components)
    aabb = _zarr_read(din, "summary/cloth_canonical_aabb_union")
    ref = r_evaluate(dout, aabb, ALL, num_points=3000)
    assert len(gpu["columns"]) == 1 + 10 + 6 + 5 + 18 + 5
    for c in gpu["columns"]:
        assert np.isnan(gpu["table"][c][1]) and np.isfinite(gpu["table"][c][[0, 2]]).all(), c
    assert_matches_restatement(gpu, ref)
    # the summary arrays, read back independently
    assert list(_zarr_read(dout, "summary/metrics/per_sample/sample_keys")) == keys
    for c in gpu["columns"]:
        assert np.array_equal(_zarr_read(dout, f"summary/metrics/per_sample/{c}"), gpu["table"][c], equal_nan=True), c
        agg = _zarr_read(dout, f"summary/metrics/aggregate/{c}")
        assert agg.shape == () and agg.dtype == np.float64 and agg == np.nanmean(gpu["table"][c]), c
    # the three output files
    cols = [""] + gpu["columns"] + ["null_percentage"]
    assert files["all_metrics.csv"].splitlines()[0].split(",") == cols
    assert [r.split(",")[0] for r in files["all_metrics_agg.csv"].splitlines()] == ["", "count", "mean", "std", "min", "25%", "50%", "75%", "max"]
    summary = json.loads(files["summary.json"])
    assert list(summary) == cols[1:] and summary["null_percentage"] == float(np.float32(1 / 3))
    # a second run writes the same files
    E.main(args + ["--output_dir", str(tmp_path / "b")])
    for f, text in files.items():
        assert open(tmp_path / "b" / f).read() == text, f


def test_device_backend_batches_and_matches_the_cpu_backend():
    rng = np.random.default_rng(4)
    be = M.DeviceBackend(DEV)
    a, b = rng.random((900, 3)), rng.random((1100, 3))
    got = be.nearest_neighbor([(a, b), (b, a), (a[:0], b), (a, b[:0])])
    want = CpuBackend().nearest_neighbor([(a, b), (b, a), (a[:0], b)])
    for (gi, gd), (wi, wd) in zip(got[:3], want):
        assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
    assert np.isinf(got[3][1]).all() and (got[3][0] == -1).all()
    v, f = sheet(10, rng)
    got = be.point_mesh_sqdist([(a, v, f), (v.astype(np.float64), v, f)])
    want = CpuBackend().point_mesh_sqdist([(a, v, f)])
    assert np.allclose(got[0][1], want[0][1], rtol=1e-12, atol=1e-18) and np.all(got[1][1] <= 1e-24)
