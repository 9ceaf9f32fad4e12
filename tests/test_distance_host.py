"""Host side of the distance, signed-distance and occupancy targets (no GPU): the numpy restatement of garmentnets_amd/distance.py against an
independent formulation (Ericson's region method, test_evaluate_host.closest_point_sqdist) and against the analytic signed distance of a box,
the three target rules on an open garment, and `python -m garmentnets_amd.prepare --backend numpy --derived_groups ...`.

Bounds.  Restatement against Ericson: |diff| <= 1e-12 * d2 + 1e-15.  Both are fp64 evaluations of the same distance with a different cancellation
(barycentric projection and clamped edges here, region selection there); measured on the 12 x 12 sheet: 3.3e-15 relative, 4.4e-16 absolute.
Box: the signed field is within ONE float32 ulp of the analytic signed distance at every node (measured: 0.49 and 0.50 ulp on the two lattices --
the fp64 error of sqrt(d2) is far below the one float32 rounding), no node lies on the box.
"""
import os

import numpy as np
import pytest

from garmentnets_amd import distance as DF
from garmentnets_amd import prepare as P
from garmentnets_amd import winding as W
from garmentnets_amd.io import zarr_store
from garmentnets_amd.io.dataset import GarmentInputDataset, read_volume
from test_evaluate_host import closest_point_sqdist, sheet
from test_winding_host import BOX_HI, BOX_LO, _chunk_mtimes, _inside, box_mesh, open_box_mesh, write_mesh_store


def _ericson(q, v, f):
    v = np.asarray(v, dtype=np.float64)
    return closest_point_sqdist(np.asarray(q, dtype=np.float64), v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])


def _held_to_ericson(q, v, f, tag):
    idx, d2 = DF.point_mesh_sqdist_reference(q, v, f)
    ref = _ericson(q, v, f)
    best = ref.min(axis=1)
    diff = np.abs(d2 - best)
    print(f"[distance] {tag}: max |diff| {diff.max():.2e}, max relative {np.max(diff / np.maximum(best, 1e-300)):.2e}")
    assert idx.dtype == np.int32 and d2.dtype == np.float64 and idx.shape == d2.shape == (len(q),)
    assert np.all(diff <= 1e-12 * best + 1e-15), tag
    # the face the restatement names is a nearest face of the independent formulation, within the same bound
    assert np.all(np.abs(ref[np.arange(len(q)), idx] - best) <= 1e-12 * best + 1e-15), tag
    return idx, d2


# ------------------------------------------------------------------------------------------------ the numpy restatement
def test_restatement_against_the_region_method_on_a_sheet():
    rng = np.random.default_rng(0)
    v, f = sheet(12, rng)
    assert len(f) == 242
    q = rng.random((500, 3)) * 1.2 - 0.1
    q[:, 2] = q[:, 2] * 0.4 - 0.2                                        # near the sheet as well as far from it
    _held_to_ericson(q, v, f, "sheet(12), 500 queries")


def test_restatement_on_degenerate_faces():
    rng = np.random.default_rng(1)
    u, a0, n = np.array([0.3, 0.5, 0.7]), np.array([0.1, 0.2, 0.3]), np.array([0.5, -0.3, 0.0])
    q = rng.random((200, 3))
    # slivers: the middle vertex lifted off the line through the other two by h |n|, from a thousandth down to the last bits
    for h in (1e-3, 1e-6, 1e-9, 1e-12, 1e-15):
        _held_to_ericson(q, np.stack([a0, a0 + 0.7 * u + h * n, a0 + 1.3 * u]), np.array([[0, 1, 2]]), f"sliver of height {h:g}")
    # h = 0: collinear up to rounding, the area is noise of either sign.  The region method then selects a region by the sign of that noise and
    # is itself wrong (it departs from the distance to the three edges by up to 1e-2 here), so this one face is held to what it is: its edges
    from test_evaluate_host import _seg_sqdist
    line = np.stack([a0, a0 + 0.7 * u, a0 + 1.3 * u])
    p, (A, B, C) = q[:, None, :], (line[[k]] for k in range(3))
    edges = np.minimum(np.minimum(_seg_sqdist(p, A, B), _seg_sqdist(p, A, C)), _seg_sqdist(p, B, C))[:, 0]
    idx, d2 = DF.point_mesh_sqdist_reference(q, line, [[0, 1, 2]])
    assert np.all(np.abs(d2 - edges) <= 1e-12 * edges + 1e-15) and not idx.any()
    v = np.stack([a0, a0 + 0.7 * u + 1e-9 * n, a0 + 1.3 * u,             # 0 1 2: a sliver
                  [0.2, 0.8, 0.1], [0.9, 0.7, 0.3],                      # 3 4
                  [0.5, 0.5, 0.5], [0.5 + 1e-9, 0.5, 0.5], [0.5, 0.5 + 1e-9, 0.5]])   # 5 6 7: a tiny face
    f = np.array([[0, 1, 2], [3, 3, 4], [4, 4, 4], [5, 6, 7], [0, 3, 4]], dtype=np.int32)      # ..., a repeated vertex, three equal vertices, ...
    for k in range(len(f)):
        _held_to_ericson(q, v, f[k:k + 1], f"face {f[k].tolist()}")
    _held_to_ericson(q, v, f, "all five")
    # exact cases: the foot of (3,3,0) on the line x=y=z is (2,2,2); a repeated vertex is its edge; three equal vertices are a point
    dv = np.array([[0, 0, 0], [1, 1, 1], [3, 3, 3], [5, 0, 0], [5, 2, 0], [9, 9, 9]], dtype=np.float64)
    for face, p, want in (([0, 1, 2], [3, 3, 0], 6.0), ([3, 3, 4], [6, 1, 0], 1.0), ([5, 5, 5], [9, 9, 10], 1.0)):
        idx, d2 = DF.point_mesh_sqdist_reference([p], dv, [face])
        assert idx[0] == 0 and d2[0] == want, (face, d2)


def test_ties_go_to_the_lowest_face_index_and_the_edge_rules():
    rng = np.random.default_rng(2)
    v, f = sheet(6, rng)
    q = rng.random((50, 3))
    idx, d2 = DF.point_mesh_sqdist_reference(q, v, f)
    # a duplicated face: the copy placed first wins every query its original won, nothing else moves
    k = int(np.bincount(idx).argmax())
    dup = np.concatenate([f[k:k + 1], f])
    idx2, d22 = DF.point_mesh_sqdist_reference(q, v, dup)
    assert np.array_equal(d22, d2) and np.array_equal(idx2, np.where(idx == k, 0, idx + 1)) and (idx2 == 0).any()
    # a query on a vertex shared by several faces: distance 0 from each of them, the lowest index is returned
    shared = 2 * 6 + 3
    on = np.flatnonzero((f == shared).any(axis=1))
    assert len(on) >= 3
    i0, z = DF.point_mesh_sqdist_reference(v[[shared]].astype(np.float64), v, f)
    assert z[0] == 0.0 and i0[0] == on.min()
    # an empty mesh, no queries, a NaN query, a face index out of range
    i, d = DF.point_mesh_sqdist_reference(q[:3], v, np.zeros((0, 3), np.int32))
    assert np.array_equal(i, [-1, -1, -1]) and np.isposinf(d).all()
    assert DF.point_mesh_sqdist_reference(np.zeros((0, 3)), v, f)[1].shape == (0,)
    i, d = DF.point_mesh_sqdist_reference([[np.nan, 0.1, 0.2], [0.1, 0.2, 0.3]], v, f)
    assert i[0] == -1 and np.isnan(d[0]) and i[1] >= 0 and np.isfinite(d[1])
    with pytest.raises(IndexError):
        DF.point_mesh_sqdist_reference(q, v, np.array([[0, 1, len(v)]]))
    with pytest.raises(ValueError):
        DF.distance_field([(v, f)], (5, 5, 5), backend="eager")
    d2f, idxf = DF.distance_field([], (5, 5, 5), backend="numpy")
    assert d2f.shape == idxf.shape == (0, 5, 5, 5)


# ------------------------------------------------------------------------------------------------ the three targets
def _box_signed_distance(pts, lo=BOX_LO, hi=BOX_HI):
    """analytic, fp64: |max(lo - p, p - hi, 0)| outside, max over the axes of (lo - p, p - hi) (negative) inside"""
    g = np.maximum(np.asarray(lo) - pts, pts - np.asarray(hi))
    return np.sqrt(np.sum(np.maximum(g, 0.0) ** 2, axis=1)) + np.minimum(g.max(axis=1), 0.0)


@pytest.mark.parametrize("shape", [(9, 9, 9), (5, 6, 7)])
def test_closed_box_fields_are_the_analytic_ones(shape):
    v, f = box_mesh()
    assert len(f) == 12
    pts = W.lattice_points(shape)
    for c in range(3):                                                   # no node lies on the box
        assert not np.isin(pts[:, c], [BOX_LO[c], BOX_HI[c]]).any()
    d2, idx = DF.distance_field_reference(v, f, shape)
    assert d2.shape == idx.shape == shape and d2.dtype == np.float64 and idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < 12
    w32 = W.winding_field_reference(v, f, shape)
    signed, dist, occ = DF.signed_distance_volume(d2, w32), DF.distance_volume(d2), DF.occupancy_volume(w32)
    assert signed.dtype == dist.dtype == occ.dtype == np.float32 and signed.shape == dist.shape == occ.shape == shape
    want = _box_signed_distance(pts).reshape(shape)
    ulp = np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)
    err = np.max(np.abs(signed.astype(np.float64) - want) / ulp)
    print(f"[distance] closed box on {shape}: signed field within {err:.2f} float32 ulp of the analytic distance")
    assert err <= 1.0
    inside = _inside(pts).reshape(shape)
    assert 0 < inside.sum() < inside.size
    assert np.array_equal(dist, np.abs(signed)) and np.array_equal(signed < 0, inside)
    assert np.array_equal(occ, inside.astype(np.float32))
    for g, vol in ((DF.DISTANCE_GROUP, dist), (DF.SIGNED_DISTANCE_GROUP, signed), (DF.OCCUPANCY_GROUP, occ)):
        assert np.array_equal(DF.derived_volume(g, d2, w32), vol)
    with pytest.raises(TypeError):
        DF.signed_distance_volume(d2, w32.astype(np.float64))


@pytest.fixture(scope="module")
def open_box_fields():
    v, f = open_box_mesh(3)
    shape = (9, 9, 9)
    d2, _ = DF.distance_field_reference(v, f, shape)
    w32 = W.winding_field_reference(v, f, shape)
    return w32, DF.signed_distance_volume(d2, w32), DF.distance_volume(d2), DF.occupancy_volume(w32)


def test_open_box_signed_field_follows_the_winding_field(open_box_fields):
    w32, signed, dist, occ = open_box_fields
    assert ((w32 > 0.2) & (w32 < 0.8)).any() and (w32 > 0.9).any() and (np.abs(w32) < 0.05).any()      # an opening, an inside, an outside
    assert np.all(dist > 0) and np.isfinite(signed).all()
    assert np.array_equal(signed <= 0, w32 >= 0.5)
    assert np.array_equal(occ, (w32 > 0.5).astype(np.float32)) and set(np.unique(occ)) == {0.0, 1.0}


def test_open_box_signed_field_is_at_most_the_distance(open_box_fields):
    """abs(signed) <= distance everywhere, exactly.  This is what the clip of the sign factor is for: the generalised winding number of an OPEN
    mesh leaves [0, 1] (outside the box, away from the opening, it is minus the solid angle of the missing patch over 4 pi), and 1 - 2 w
    exceeds 1 where w < 0.  On this mesh and lattice w32 lies in [-0.0641, 0.9997]; unclipped, 305 of the 729 nodes would exceed the distance,
    by a factor of up to 1.128 (= 1 - 2 min w).  Where w32 lies in [0, 1] the field is float32((1 - 2 w32) * distance), unclipped."""
    w32, signed, dist, _ = open_box_fields
    over = w32 < 0
    print(f"[distance] open box: w32 in [{w32.min():.4f}, {w32.max():.4f}], the clip is live at {int(over.sum())} of {over.size} nodes, "
          f"largest |signed| / distance {float((np.abs(signed) / dist).max()):.4f}")
    assert over.any() and w32.max() <= 1                                 # the case is live: without the clip these nodes pass the distance
    assert np.all(np.abs(signed) <= dist) and np.array_equal(signed[over], dist[over])
    d64 = np.sqrt(DF.distance_field_reference(*open_box_mesh(3), (9, 9, 9))[0])
    assert np.array_equal(signed[~over], ((1.0 - 2.0 * w32.astype(np.float64)) * d64).astype(np.float32)[~over])


# ------------------------------------------------------------------------------------------------ prepare, numpy backend
SIZE = 5
ALL = list(P.DERIVED_GROUPS)


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    store = tmp_path_factory.mktemp("distance") / "ds.zarr"
    meshes = [open_box_mesh(s, drop=s % 4) for s in range(3)]
    keys = write_mesh_store(store, meshes, mc_stand_in=True)
    first = P.prepare_store(str(store), volume_size=SIZE, backend="numpy", batch_size=2, log=lambda row: None)
    rows = []
    summary = P.prepare_store(str(store), volume_size=SIZE, groups=[], backend="numpy", batch_size=2, log=rows.append, derived_groups=ALL)
    return str(store), keys, meshes, rows, summary, first


def test_prepare_writes_the_three_derived_groups(prepared):
    store, keys, meshes, rows, summary, first = prepared
    assert P.DERIVED_GROUPS == ("nocs_distance_field", "nocs_signed_distance_field", "nocs_occupancy_grid")
    assert first["written"] == {g: 3 for g in P.GROUPS}                  # a run without --derived_groups: today's dict
    assert summary["samples"] == 3 and summary["written"] == {g: 3 for g in ALL}
    assert [r["sample"] for r in rows[:-1]] == keys and all(r["written"] == ALL for r in rows[:-1])
    samples = zarr_store.open_group(store, create=False)["samples"]
    for key, (nocs, faces) in zip(keys, meshes):
        vol = samples[key]["volume"]
        for g in ALL:
            assert vol[g].array_meta(str(SIZE)) == ((SIZE,) * 3, np.dtype(np.float32))
        w32 = vol["nocs_winding_number_field"][str(SIZE)][:]
        d2, _ = DF.distance_field_reference(nocs.astype(np.float64), faces, (SIZE,) * 3)
        assert np.array_equal(vol["nocs_distance_field"][str(SIZE)][:], DF.distance_volume(d2))
        assert np.array_equal(vol["nocs_signed_distance_field"][str(SIZE)][:], DF.signed_distance_volume(d2, w32))
        assert np.array_equal(vol["nocs_occupancy_grid"][str(SIZE)][:], DF.occupancy_volume(w32))
        assert vol["nocs_signed_distance_field"][str(SIZE)][:][2, 2, 2] < 0 < vol["nocs_signed_distance_field"][str(SIZE)][:][0, 0, 0]


def test_dataset_reads_the_derived_groups(prepared):
    store = prepared[0]
    kw = dict(num_pc_sample=100, volume_size=SIZE, num_volume_sample=200, num_surface_sample=40, static_epoch_seed=True)
    tsdf = GarmentInputDataset(store, volume_group="nocs_signed_distance_field", tsdf_clip_value=0.05, **kw)
    occ = GarmentInputDataset(store, volume_group="nocs_occupancy_grid", **kw)
    for i in range(3):
        clipped = read_volume(tsdf.samples_group[tsdf.keys[i]], "nocs_signed_distance_field", SIZE, 0.05)
        assert np.isfinite(clipped).all() and clipped.min() == -1.0 and clipped.max() == 1.0
        t = tsdf[i]["gt_volume_value"]
        # a trilinear sample of values in [-1, 1]: eight fp32 weights that sum to 1 within a few ulp
        assert t.shape == (1, 200) and np.isfinite(t).all() and np.abs(t).max() <= 1.0 + 8 * 2.0 ** -23 and t.min() < 0 < t.max()
        o = occ[i]["gt_volume_value"]
        assert o.shape == (1, 200) and set(np.unique(o)) == {0.0, 1.0}
    dist = GarmentInputDataset(store, volume_group="nocs_distance_field", volume_absolute_value=True, **kw)
    assert np.isfinite(dist[0]["gt_volume_value"]).all() and dist[0]["gt_volume_value"].min() >= 0


def test_second_run_keeps_what_is_there_and_overwrite_rebuilds_one_group(prepared):
    store = prepared[0]
    before = _chunk_mtimes(store)
    args = ["--zarr_in", store, "--volume_size", str(SIZE), "--backend", "numpy"]
    again = P.main(args + ["--derived_groups"] + ALL)
    assert again["written"] == {g: 0 for g in list(P.GROUPS) + ALL} and _chunk_mtimes(store) == before
    plain = P.main(args)
    assert plain["written"] == {g: 0 for g in P.GROUPS} and _chunk_mtimes(store) == before
    one = P.main(args + ["--groups", "--derived_groups", "nocs_occupancy_grid", "--overwrite"])
    assert one["written"] == {"nocs_occupancy_grid": 3}
    after = _chunk_mtimes(store)
    changed = {p for p in after if after[p] != before.get(p)}
    assert changed and all(os.sep + "nocs_occupancy_grid" + os.sep in p for p in changed)


def test_derived_group_errors(tmp_path, capsys):
    store = tmp_path / "ds.zarr"
    keys = write_mesh_store(store, [box_mesh()])
    # the signed field and the occupancy grid read the winding field: absent and not built in the same run
    for g in ("nocs_signed_distance_field", "nocs_occupancy_grid"):
        with pytest.raises(ValueError, match="nocs_winding_number_field/5"):
            P.prepare_store(str(store), volume_size=5, groups=[], backend="numpy", derived_groups=[g], log=lambda row: None)
    only = P.prepare_store(str(store), volume_size=5, groups=[], backend="numpy", derived_groups=["nocs_distance_field"], log=lambda row: None)
    assert only["written"] == {"nocs_distance_field": 1}                 # the distance alone needs no winding field
    both = P.prepare_store(str(store), volume_size=5, groups=["nocs_winding_number_field"], backend="numpy",
                           derived_groups=["nocs_signed_distance_field"], log=lambda row: None)        # built in the same run
    assert both["written"] == {"nocs_winding_number_field": 1, "nocs_signed_distance_field": 1}
    with pytest.raises(SystemExit):
        P.main(["--zarr_in", str(store), "--volume_size", "5", "--backend", "numpy", "--derived_groups", "tsdf"])
    assert "tsdf" in capsys.readouterr().err
    with pytest.raises(ValueError, match="unknown derived group"):
        P.prepare_store(str(store), volume_size=5, backend="numpy", derived_groups=["nocs_winding_number_field"])
    with pytest.raises(SystemExit):                                      # --groups still refuses a derived group, naming it
        P.main(["--zarr_in", str(store), "--volume_size", "5", "--backend", "numpy", "--groups", "nocs_occupancy_grid"])
    assert "nocs_occupancy_grid" in capsys.readouterr().err
    assert P.build_parser().parse_args(["--zarr_in", "x"]).derived_groups == []
    # a mesh without faces: refused, naming the sample
    empty = tmp_path / "empty.zarr"
    keys = write_mesh_store(empty, [box_mesh()])
    mesh = zarr_store.open_group(str(empty), create=False)["samples"][keys[0]]["mesh"]
    mesh.array("cloth_faces_tri", np.zeros((0, 3), dtype=np.int32))
    with pytest.raises(ValueError, match=keys[0]):
        P.prepare_store(str(empty), volume_size=5, groups=[], backend="numpy", derived_groups=["nocs_distance_field"], log=lambda row: None)
