"""GPU (-m gpu): the winding-number kernels of csrc/winding.hip (ops.winding_number*, ops.winding_field_batch) against the numpy restatement of
garmentnets_amd/winding.py, and `python -m garmentnets_amd.prepare` end to end.

Tolerance: |w_dev - w_ref| <= F * 2**-50 absolute, F the faces of the mesh.  Both sides evaluate the two arguments of atan2 with the same separately
rounded operations, so those agree bit for bit; what can differ is atan2 itself (a few ulp of a term of at most 2 pi, i.e. a few 1e-16 of w per face)
and the roundings of the running sum that follow from it, both linear in F as the faces are added in the same order.  F = 0 therefore demands equality.
No case is left out of a comparison: the inputs are generic (seeded jitter on every vertex of a bumpy sheet, seeded random queries), and the bound does
not depend on how close a query is to the surface, because the conditioning of atan2's arguments is shared by both sides.

Shapes: F in {0, 1, tile - 1, tile, tile + 1, 1922} with the tile of 128 faces; 1, 63 and 1025 queries (a workgroup owns 1024); lattices (5, 6, 9), 9^3
and 17^3; a ragged batch of three meshes with the empty one; zero-area faces; queries on vertices.

Measured on an MI355X: see DESIGN.md, "Winding numbers".
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import ops, prepare as P, train_pipeline as TP, winding as W  # noqa: E402
from garmentnets_amd.io import zarr_store  # noqa: E402
from garmentnets_amd.io.dataset import TARGET_FIELDS, GarmentInputDataset  # noqa: E402
from garmentnets_amd.io.resident import ResidentDataset  # noqa: E402
from test_train_pipeline_host import small_model  # noqa: E402
from test_winding_host import box_mesh, open_box_mesh, write_mesh_store  # noqa: E402

DEV = "cuda:0"
TILE, SPAN = 128, 1024                      # WN_TILE, WN_BLOCK * WN_QPT of csrc/winding.hip
FACE_COUNTS = (0, 1, TILE - 1, TILE, TILE + 1, 1922)
QUERY_COUNTS = (1, 63, SPAN + 1)
LATTICES = ((5, 6, 9), (9, 9, 9), (17, 17, 17))


def tol(nf):
    return nf * 2.0 ** -50


def sheet_mesh(n=32, seed=5):
    """an n x n bumpy open sheet across the unit cube, every vertex jittered: 2 (n-1)^2 = 1922 faces"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(0.07, 0.93, n), np.linspace(0.06, 0.94, n), indexing="ij")
    z = 0.5 + 0.17 * np.sin(5.1 * u) * np.cos(4.3 * v)
    verts = np.stack([u, v, z], axis=-1).reshape(-1, 3) + rng.uniform(-3e-3, 3e-3, (n * n, 3))
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], axis=1).reshape(-1, 3).astype(np.int32)
    return verts, faces


def _d(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _mesh(v, f):
    return _d(v), _d(f, torch.int32)


def _close(got, want, nf, tag):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64, (tag, got.shape, got.dtype)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    print(f"[winding] {tag}: max |dev - ref| {err:.3e}, bound {tol(nf):.3e}")
    assert np.isfinite(got).all() and err <= tol(nf), (tag, err, tol(nf))
    return err


@pytest.fixture(scope="module")
def sheet():
    """the sheet, 1025 seeded queries and the reference of every face count at them; the lattice references -- computed once"""
    v, f = sheet_mesh()
    assert len(f) == 1922
    q = np.random.default_rng(11).random((SPAN + 1, 3))
    ref = {nf: W.winding_number_reference(q, v, f[:nf]) for nf in FACE_COUNTS}
    lat = {shape: W.winding_number_reference(W.lattice_points(shape), v, f) for shape in LATTICES}
    assert np.abs(ref[1922]).max() > 0.3 and np.abs(lat[(9, 9, 9)]).max() > 0.3
    return dict(v=v, f=f, q=q, ref=ref, lat=lat)


# ------------------------------------------------------------------------------------------------ points
@pytest.mark.parametrize("nq", QUERY_COUNTS)
@pytest.mark.parametrize("nf", FACE_COUNTS)
def test_number_matches_the_reference(sheet, nf, nq):
    got = ops.winding_number(_d(sheet["q"][:nq]), *_mesh(sheet["v"], sheet["f"][:nf]))
    _close(got, sheet["ref"][nf][:nq], nf, f"F={nf} nq={nq}")


def test_zero_area_faces_and_queries_on_vertices(sheet):
    v, f = sheet["v"], sheet["f"][:300].copy()
    f[10:20, 1] = f[10:20, 0]                                            # (v0, v0, v2)
    f[40:45, 2] = f[40:45, 1]                                            # (v0, v1, v1)
    f[50] = f[50, 0]                                                     # a point
    q = np.concatenate([v[[0, 17, 33, 500, 1023]], v[f[12]], sheet["q"][:40]])      # mesh vertices, those of a zero-area face, generic points
    want = W.winding_number_reference(q, v, f)
    assert np.isfinite(want).all()
    _close(ops.winding_number(_d(q), _d(v), _d(f, torch.int64)), want, len(f), "zero-area faces, queries on vertices")


def test_ragged_batch_with_an_empty_mesh(sheet):
    bv, bf = box_mesh()
    meshes = [(sheet["v"], sheet["f"]), (np.zeros((0, 3)), np.zeros((0, 3), np.int32)), (bv, bf), (sheet["v"], sheet["f"][:TILE + 1])]
    queries = [sheet["q"][:700], sheet["q"][:5], sheet["q"][100:1125], np.zeros((0, 3))]
    got = ops.winding_number_batch([_d(q) for q in queries], [_mesh(v, f) for v, f in meshes])
    assert len(got) == 4 and got[3].shape == (0,)
    _close(got[0], sheet["ref"][1922][:700], 1922, "batch: sheet")
    assert torch.equal(got[1].cpu(), torch.zeros(5, dtype=torch.float64))
    _close(got[2], W.winding_number_reference(queries[2], bv, bf), 12, "batch: box")
    shape = (5, 6, 9)
    field = ops.winding_field_batch([_mesh(v, f) for v, f in meshes[:3]], shape)
    assert field.shape == (3,) + shape and field.dtype == torch.float32
    assert torch.equal(field[1].cpu(), torch.zeros(shape))
    want = W.winding_field_reference(bv, bf, shape)
    # each side rounds to float32 once: half an ulp each, an ulp <= 2**-23 below 2
    assert float(np.abs(field[2].cpu().numpy().astype(np.float64) - want).max()) <= tol(12) + 2.0 ** -23


def test_pure_function_of_query_and_mesh(sheet):
    mesh, other = _mesh(sheet["v"], sheet["f"]), _mesh(*box_mesh())
    q = _d(sheet["q"][:300])
    alone = ops.winding_number(q, *mesh)
    assert torch.equal(alone, ops.winding_number(q, *mesh))                                       # two identical calls
    filler = _d(sheet["q"][300:])
    inside = ops.winding_number_batch([filler, _d(sheet["q"][:37]), q, filler[:3]], [other, other, mesh, mesh])
    assert torch.equal(alone, inside[2])                                                          # another offset, other pairs around it
    assert torch.equal(alone[:37], ops.winding_number(_d(sheet["q"][:37]), *mesh))                # another launch geometry


# ------------------------------------------------------------------------------------------------ the lattice
@pytest.mark.parametrize("shape", LATTICES)
def test_field_is_the_numbers_at_the_lattice_points(sheet, shape):
    mesh = _mesh(sheet["v"], sheet["f"])
    pts = ops.winding_number(_d(W.lattice_points(shape)), *mesh)
    _close(pts, sheet["lat"][shape], 1922, f"lattice {shape}")
    field = ops.winding_field_batch([mesh], shape)
    assert field.shape == (1,) + shape and field.dtype == torch.float32
    assert torch.equal(field.reshape(-1).view(torch.int32), pts.float().view(torch.int32))        # bit for bit
    via_module = W.winding_field([(sheet["v"], sheet["f"])], shape)
    assert via_module.dtype == np.float32 and np.array_equal(via_module, field.cpu().numpy())


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_face_index_raises_and_leaves_the_next_call_alone(sheet):
    mesh = _mesh(sheet["v"], sheet["f"][:200])
    q = _d(sheet["q"][:63])
    before = ops.winding_number(q, *mesh)
    bad = sheet["f"][:200].copy()
    bad[150, 1] = len(sheet["v"])
    with pytest.raises(IndexError):
        ops.winding_number(q, _d(sheet["v"]), _d(bad, torch.int32))
    bad[150, 1] = -1
    with pytest.raises(IndexError):
        ops.winding_field_batch([mesh, (_d(sheet["v"]), _d(bad, torch.int32))], (5, 5, 5))
    with pytest.raises(IndexError):                                                               # a pair without queries still has its faces checked
        ops.winding_number_batch([q[:0]], [(_d(sheet["v"]), _d(bad.astype(np.int64) + 2 ** 33, torch.int64))])
    assert torch.equal(before, ops.winding_number(q, *mesh))


def test_limits_are_refused_by_name(sheet):
    mesh = _mesh(sheet["v"], sheet["f"][:4])
    with pytest.raises(ValueError, match="gn_winding_field_batch"):
        ops.winding_field_batch([mesh], (1, 5, 5))
    with pytest.raises(ValueError):
        ops.winding_number_batch([_d(sheet["q"][:3])], [])
    with pytest.raises(ValueError):
        ops.winding_number(_d(sheet["q"][:3, :2]), *mesh)
    with pytest.raises(TypeError):
        ops.winding_number(_d(sheet["q"][:3]), mesh[0], mesh[1].double())


# ------------------------------------------------------------------------------------------------ prepare, end to end
def test_prepare_end_to_end_then_resident_batches_and_a_training_step(tmp_path):
    size = 9
    store = str(tmp_path / "ds.zarr")
    meshes = [open_box_mesh(s, drop=s) for s in range(3)]
    keys = write_mesh_store(store, meshes)
    summary = P.main(["--zarr_in", store, "--volume_size", str(size), "--marching_cubes", "--batch_size", "2"])
    assert summary["written"] == {g: 3 for g in P.GROUPS + ("marching_cube_mesh",)}
    samples = zarr_store.open_group(store, create=False)["samples"]
    for key, (nocs, faces) in zip(keys, meshes):
        field = samples[key]["volume"]["nocs_winding_number_field"][str(size)][:]
        assert field.shape == (size,) * 3 and field.dtype == np.float32
        assert np.abs(field.astype(np.float64) - W.winding_field_reference(nocs, faces, (size,) * 3)).max() <= tol(len(faces)) + 2.0 ** -23
        # near 1 deep inside, near 0 outside, in between at the opening
        assert field[4, 4, 4] > 0.9 and abs(field[0, 0, 0]) < 0.05 and ((field > 0.2) & (field < 0.8)).any()
        mc = samples[key]["marching_cube_mesh"]
        mv, mf, on = mc["marching_cube_verts"][:], mc["marching_cube_faces"][:], mc["is_vertex_on_surface"][:]
        assert (mv.dtype, mf.dtype, on.dtype) == (np.float32, np.int32, np.bool_)
        assert len(mv) > 0 and len(mf) > 0 and on.shape == (len(mv),) and mf.min() >= 0 and mf.max() < len(mv)
        print(f"[winding] {key}: centre {field[4, 4, 4]:.4f}, {len(mv)} marching-cubes vertices, {int(on.sum())} on the surface")
        assert on.any() and not on.all()
        assert mc.attrs["empty"] is False and mc.attrs["on_surface_distance"] == 1.0 / (size - 1)
    again = P.main(["--zarr_in", store, "--volume_size", str(size), "--marching_cubes"])
    assert not any(again["written"].values())
    # the store now feeds the training loops: the resident dataset yields the host dataset's batches
    ds = GarmentInputDataset(store, num_pc_sample=200, volume_size=size, num_volume_sample=96, num_surface_sample=80, num_mc_surface_sample=64,
                             static_epoch_seed=True, enable_augumentation=False)
    chunk = [2, 0, 1]
    host = GarmentInputDataset.collate([ds[k] for k in chunk])
    got = ResidentDataset(ds, [0, 1, 2], DEV).batch(chunk)
    for k in TARGET_FIELDS:
        assert torch.equal(getattr(got, k).cpu(), getattr(host, k)), k
    assert 0.0 < float(got.is_query_point_on_surf.mean()) < 1.0 and float(got.gt_volume_value.max()) > 0.9
    model = small_model(1, planted_nocs=True, reduce_method="max", mc=0.5).to(DEV).requires_grad_(True).train()
    metrics = TP.train_step(model, model.configure_optimizers(), got)
    assert set(metrics) == {"loss", "volume_loss", "surface_loss", "mc_surface_loss"} and all(math.isfinite(v) for v in metrics.values())


def test_prepare_writes_an_empty_mesh_when_the_level_is_out_of_range(tmp_path):
    store = str(tmp_path / "far.zarr")
    v, f = open_box_mesh(0)
    keys = write_mesh_store(store, [((v - 0.5) * 0.01 + 0.5, f[:2])])                 # two tiny faces: the field stays far below 0.5
    P.main(["--zarr_in", store, "--volume_size", "5", "--marching_cubes", "--groups", "nocs_winding_number_field"])
    mc = zarr_store.open_group(store, create=False)["samples"][keys[0]]["marching_cube_mesh"]
    assert mc["marching_cube_verts"][:].shape == (0, 3) and mc["marching_cube_faces"][:].shape == (0, 3) and mc["is_vertex_on_surface"][:].shape == (0,)
    assert mc["marching_cube_faces"][:].dtype == np.int32 and "range" in mc.attrs["empty"]
