"""Host side of the winding-number targets (no GPU): the numpy restatement of garmentnets_amd/winding.py against what a winding number must be
(1 inside a closed outward-oriented surface, 0 outside, odd in the orientation, additive over meshes, finite on a vertex), and
`python -m garmentnets_amd.prepare --backend numpy` on a store that holds meshes and point clouds but no targets.

The bounds on the closed box are those of the definition in fp64: 12 faces, each term a few ulp of at most 2 pi, so |w - 1| and |w| stay far
below 1e-14 (measured: 7e-16 inside, 1.3e-16 outside); no lattice node lies in a face plane.

The package has no host marching cubes (common.marching_cubes_util runs on the device), so `--marching_cubes` is covered by
tests/test_gpu_winding.py; here the store carries a hand-made marching_cube_mesh group, which also shows that a run without the flag leaves it alone.

The mesh and store builders below are shared with tests/test_gpu_winding.py.
"""
import os

import numpy as np
import pytest

from garmentnets_amd import prepare as P
from garmentnets_amd import winding as W
from garmentnets_amd.io import zarr_store
from garmentnets_amd.io.dataset import TARGET_FIELDS, TASK_SPACE_VOLUME_GROUP, AABBGripNormalizer, GarmentInputDataset

BOX_LO, BOX_HI = (.2301, .2203, .2107), (.7707, .7809, .7611)
AABB = np.array([[-0.4, -0.4, -0.9], [0.4, 0.4, 0.05]], dtype=np.float32)
# the six sides of a box as quads of corner (ix, iy, iz) -> 4 ix + 2 iy + iz, counter-clockwise seen from outside
BOX_QUADS = ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3))


def box_mesh(lo=BOX_LO, hi=BOX_HI):
    """the closed box: 8 vertices, 12 outward faces"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    verts = np.array([[(lo, hi)[ix][0], (lo, hi)[iy][1], (lo, hi)[iz][2]] for ix in (0, 1) for iy in (0, 1) for iz in (0, 1)])
    faces = np.array([t for q in BOX_QUADS for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int32)
    return verts, faces


def open_box_mesh(seed, lo=0.1, hi=0.9, n=2, jitter=0.01, drop=0):
    """a closed-ish garment: a box whose sides are n x n quads, every vertex jittered, with ONE face pair (quad number `drop` of the z = hi
    side) removed.  Outward faces."""
    rng = np.random.default_rng(seed)
    ax = np.linspace(lo, hi, n + 1)
    index, verts, faces = {}, [], []

    def vid(i, j, k):
        if (i, j, k) not in index:
            index[(i, j, k)] = len(verts)
            verts.append([ax[i], ax[j], ax[k]])
        return index[(i, j, k)]
    for axis in range(3):
        for side in (0, n):
            for u in range(n):
                for v in range(n):
                    def corner(du, dv):
                        c = [0, 0, 0]
                        c[axis], c[(axis + 1) % 3], c[(axis + 2) % 3] = side, u + du, v + dv
                        return vid(*c)
                    q = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]        # (axis+1) x (axis+2) = +axis: outward on the far side
                    if side == 0:
                        q = q[::-1]
                    if axis == 2 and side == n and u * n + v == drop:
                        continue
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    verts = np.asarray(verts, dtype=np.float64) + rng.uniform(-jitter, jitter, (len(verts), 3))
    return verts.astype(np.float32), np.asarray(faces, dtype=np.int32)


def write_mesh_store(path, meshes, seed=0, views=(60, 60, 60, 60), mc_stand_in=False):
    """a dataset store in the reference's layout with everything BUT the targets prepare builds: point_cloud/*, mesh/*, attrs,
    summary/cloth_aabb_union.  meshes: [(nocs verts, faces)]; the simulation-space mesh is an affine image of the NOCS one inside the
    store's bounding box, the cloud random points of the faces with random colours.  mc_stand_in: also a hand-made marching_cube_mesh group."""
    rng = np.random.default_rng(seed)
    root = zarr_store.open_group(str(path))
    root.require_group("summary").array("cloth_aabb_union", AABB)
    keys = []
    for i, (nocs, faces) in enumerate(meshes):
        key = f"{i:05d}_Dress_{i:06d}_0"
        keys.append(key)
        sg = root.require_group("samples").require_group(key)
        sg.put_attrs({"scale": 1.0 + 0.1 * i, "sample_id": f"{i:05d}_Dress", "garment_name": "Dress", "grip_vertex_idx": i % len(nocs)})
        nocs = np.asarray(nocs, dtype=np.float32)
        sim = ((nocs - 0.5) * np.float32([0.7, 0.7, 0.9]) + np.float32([0.0, 0.0, -0.43])).astype(np.float32)
        n = sum(views)
        bc = rng.dirichlet((1, 1, 1), n).astype(np.float32)
        tri = faces[rng.integers(0, len(faces), n)]
        on = lambda v: np.einsum("nk,nkc->nc", bc, v[tri]).astype(np.float32)
        pc, mesh = sg.require_group("point_cloud"), sg.require_group("mesh")
        pc.array("point", on(sim))
        pc.array("nocs", on(nocs))
        pc.array("rgb", rng.integers(0, 256, (n, 3)).astype(np.uint8))
        pc.array("sizes", np.array(views, dtype=np.int64))
        mesh.array("cloth_verts", sim)
        mesh.array("cloth_nocs_verts", nocs)
        mesh.array("cloth_faces_tri", np.asarray(faces, dtype=np.int32))
        if mc_stand_in:
            mc = sg.require_group("marching_cube_mesh")
            mc.array("marching_cube_verts", nocs)
            mc.array("marching_cube_faces", np.asarray(faces, dtype=np.int32))
            mc.array("is_vertex_on_surface", rng.random(len(nocs)) > 0.4)
    return keys


def _inside(points, lo=BOX_LO, hi=BOX_HI):
    return np.all((points > np.asarray(lo)) & (points < np.asarray(hi)), axis=1)


# ------------------------------------------------------------------------------------------------ the numpy reference
@pytest.fixture(scope="module")
def box_field():
    v, f = box_mesh()
    pts = W.lattice_points((9, 9, 9))
    return v, f, pts, W.winding_number_reference(pts, v, f)


def test_closed_box_is_one_inside_and_zero_outside(box_field):
    v, f, pts, w = box_field
    inside = _inside(pts)
    assert 0 < inside.sum() < len(pts) and len(f) == 12
    for c in range(3):                                                   # no node lies in a face plane
        assert not np.isin(pts[:, c], [BOX_LO[c], BOX_HI[c]]).any()
    err_in, err_out = np.abs(w[inside] - 1).max(), np.abs(w[~inside]).max()
    print(f"[winding] closed box on 9^3: |w - 1| inside {err_in:.2e}, |w| outside {err_out:.2e}")
    assert err_in < 1e-14 and err_out < 1e-14
    field = W.winding_field_reference(v, f, (9, 9, 9))
    assert field.dtype == np.float32 and field.shape == (9, 9, 9) and np.array_equal(field.reshape(-1), w.astype(np.float32))


def test_lattice_is_the_grid_sample_convention():
    pts = W.lattice_points((5, 6, 9)).reshape(5, 6, 9, 3)
    assert pts[2, 3, 7].tolist() == [2 / 4, 3 / 5, 7 / 8] and pts[4, 5, 8].tolist() == [1.0, 1.0, 1.0] and pts[0, 0, 0].tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        W.lattice_points((5, 1, 9))


def test_flipped_faces_negate_the_field(box_field):
    v, f, pts, w = box_field
    flipped = W.winding_number_reference(pts, v, f[:, ::-1])             # (v2, v1, v0): the same triple product and norms in another order
    assert np.abs(flipped + w).max() < 2e-14 and np.abs(flipped).max() > 0.99


def test_concatenated_meshes_add(box_field):
    v, f, pts, w = box_field
    v2, f2 = open_box_mesh(3)
    w2 = W.winding_number_reference(pts, v2, f2)
    both = W.winding_number_reference(pts, np.concatenate([v, v2.astype(np.float64)]), np.concatenate([f, f2 + len(v)]))
    assert np.abs(both - (w + w2)).max() < (len(f) + len(f2)) * 2.0 ** -50          # the same terms, summed in another grouping
    assert np.abs(w2).max() > 0.5


def test_query_on_a_vertex_is_finite_and_empty_mesh_is_zero(box_field):
    v, f, pts, _ = box_field
    w = W.winding_number_reference(v, v, f)
    assert np.isfinite(w).all()
    assert np.array_equal(W.winding_number_reference(pts, v, np.zeros((0, 3), np.int32)), np.zeros(len(pts)))
    assert W.winding_number_reference(np.zeros((0, 3)), v, f).shape == (0,)
    with pytest.raises(IndexError):
        W.winding_number_reference(pts, v, np.array([[0, 1, 8]]))
    with pytest.raises(ValueError):
        W.winding_field([(v, f)], (5, 5, 5), backend="eager")


# ------------------------------------------------------------------------------------------------ prepare, numpy backend
SIZE = 5


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    store = tmp_path_factory.mktemp("winding") / "ds.zarr"
    meshes = [open_box_mesh(s, drop=s % 4) for s in range(3)]
    keys = write_mesh_store(store, meshes, mc_stand_in=True)
    rows = []
    summary = P.prepare_store(str(store), volume_size=SIZE, backend="numpy", batch_size=2, log=rows.append)
    return str(store), keys, meshes, rows, summary


def test_prepare_writes_both_volume_groups(prepared):
    store, keys, meshes, rows, summary = prepared
    assert summary["samples"] == 3 and summary["written"] == {"nocs_winding_number_field": 3, TASK_SPACE_VOLUME_GROUP: 3}
    assert [r["sample"] for r in rows[:-1]] == keys and all(r["seconds"] > 0 for r in rows)
    samples = zarr_store.open_group(store, create=False)["samples"]
    for key, (nocs, faces) in zip(keys, meshes):
        for g in P.GROUPS:
            assert samples[key]["volume"][g].array_meta(str(SIZE)) == ((SIZE,) * 3, np.dtype(np.float32))
        got = samples[key]["volume"]["nocs_winding_number_field"][str(SIZE)][:]
        assert np.array_equal(got, W.winding_field_reference(nocs, faces, (SIZE,) * 3))
        assert got[2, 2, 2] > 0.9 and abs(got[0, 0, 0]) < 0.05                        # the box centre is inside, the cube corner outside
        # the task-space field is the field of exactly the vertices the dataset queries in task space
        task = AABBGripNormalizer(AABB)(samples[key]["mesh"]["cloth_verts"][:])
        assert np.array_equal(samples[key]["volume"][TASK_SPACE_VOLUME_GROUP][str(SIZE)][:], W.winding_field_reference(task, faces, (SIZE,) * 3))


def test_dataset_reads_every_target_from_the_prepared_store(prepared):
    store = prepared[0]
    ds = GarmentInputDataset(store, num_pc_sample=100, volume_size=SIZE, num_volume_sample=50, num_surface_sample=40, num_mc_surface_sample=30,
                             static_epoch_seed=True)
    for i in range(3):
        s = ds[i]
        assert set(TARGET_FIELDS) <= set(s)
        assert s["volume_query_points"].shape == (1, 50, 3) and s["gt_volume_value"].shape == (1, 50) and s["surf_query_points"].shape == (1, 40, 3)
        assert np.isfinite(s["gt_volume_value"]).all() and s["gt_volume_value"].max() > 0.5 > s["gt_volume_value"].min()
    task = GarmentInputDataset(store, num_pc_sample=100, volume_size=SIZE, num_volume_sample=50, num_surface_sample=40, static_epoch_seed=True,
                               volume_group=TASK_SPACE_VOLUME_GROUP)
    assert np.isfinite(task[1]["gt_volume_value"]).all()


def _chunk_mtimes(store):
    out = {}
    for d, _, files in os.walk(store):
        for f in files:
            out[os.path.join(d, f)] = os.stat(os.path.join(d, f)).st_mtime_ns
    return out


def test_second_run_keeps_what_is_there_and_overwrite_rebuilds(prepared):
    store = prepared[0]
    before = _chunk_mtimes(store)
    again = P.main(["--zarr_in", store, "--volume_size", str(SIZE), "--backend", "numpy"])
    assert again["written"] == {g: 0 for g in P.GROUPS} and _chunk_mtimes(store) == before
    one = P.main(["--zarr_in", store, "--volume_size", str(SIZE), "--backend", "numpy", "--groups", "nocs_winding_number_field", "--overwrite"])
    assert one["written"] == {"nocs_winding_number_field": 3}
    after = _chunk_mtimes(store)
    changed = {p for p in after if after[p] != before.get(p)}
    assert changed and all(os.sep + "nocs_winding_number_field" + os.sep in p for p in changed)       # the mc stand-in, the other group: untouched


def test_argument_errors(tmp_path, capsys):
    store = tmp_path / "ds.zarr"
    write_mesh_store(store, [box_mesh()])
    with pytest.raises(SystemExit):
        P.main(["--zarr_in", str(store), "--volume_size", "5", "--backend", "numpy", "--groups", "nocs_occupancy_grid"])
    assert "nocs_occupancy_grid" in capsys.readouterr().err
    with pytest.raises(ValueError, match="unknown volume group"):
        P.prepare_store(str(store), volume_size=5, groups=["tsdf"], backend="numpy")
    with pytest.raises(SystemExit):
        P.main(["--zarr_in", str(store), "--backend", "eager"])
    bare = tmp_path / "bare.zarr"
    zarr_store.open_group(str(bare)).require_group("samples").require_group("00000_Dress_000000_0").require_group("point_cloud")
    with pytest.raises(ValueError, match="mesh/cloth_verts"):
        P.prepare_store(str(bare), volume_size=5, backend="numpy")
    with pytest.raises(ValueError, match="no samples"):
        P.prepare_store(str(tmp_path / "nothing.zarr"), volume_size=5, backend="numpy")
    a = P.build_parser().parse_args(["--zarr_in", "x"])
    assert (a.volume_size, a.groups, a.marching_cubes, a.on_surface_distance, a.overwrite, a.backend) == \
        (128, list(P.GROUPS), False, None, False, "hip")
