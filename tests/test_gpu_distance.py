"""GPU (-m gpu): the lattice distance kernel of csrc/eval_dist.hip (ops.distance_field_batch) against the kernel it shares its arithmetic with
(ops.point_mesh_sqdist_batch at winding.lattice_points) and against the numpy restatement of garmentnets_amd/distance.py, and
`python -m garmentnets_amd.prepare --derived_groups` with both backends, whose store then feeds the resident dataset and a training step with
volume_group = nocs_signed_distance_field (tsdf_clip_value 0.05) and nocs_occupancy_grid.

Every comparison is for EQUALITY, in the face index and in the bits of d2: the library is built with -ffp-contract=off, every operation of the
definition is one IEEE operation on both sides, and each node scans the faces in index order with a strict `<`.

Shapes: F in {1, tile - 1, tile, tile + 1} with the staging tile of 128 faces, and 1922 faces (16 tiles); lattices (2, 2, 2), (5, 6, 7) and
(11, 11, 11) -- 1331 nodes: one full workgroup span of 1024 (256 threads x 4 nodes) and a ragged one -- and 17^3 (four full spans and a tail).
"""
import math
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import distance as DF, ops, prepare as P, train_pipeline as TP, winding as W  # noqa: E402
from garmentnets_amd.io import zarr_store  # noqa: E402
from garmentnets_amd.io.dataset import GarmentInputDataset  # noqa: E402
from garmentnets_amd.io.resident import ResidentDataset  # noqa: E402
from test_evaluate_host import sheet  # noqa: E402
from test_train_pipeline_host import small_model  # noqa: E402
from test_winding_host import open_box_mesh, write_mesh_store  # noqa: E402

DEV = "cuda:0"
TILE, SPAN = 128, 1024                      # PM_TILE, ED_BLOCK * DF_QPT of csrc/eval_dist.hip
FACE_COUNTS = (1, TILE - 1, TILE, TILE + 1)
LATTICES = ((2, 2, 2), (5, 6, 7), (11, 11, 11))
assert SPAN < 11 ** 3 < 2 * SPAN and 11 ** 3 % SPAN


def _d(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _mesh(v, f):
    return _d(v), _d(f, torch.int32)


def _at_lattice_points(v, f, shape):
    """the existing kernel at the uploaded lattice points -> (d2, face_idx) shaped like the volume"""
    idx, d2 = ops.point_mesh_sqdist(_d(W.lattice_points(shape)), *_mesh(v, f))
    return d2.reshape(shape), idx.reshape(shape)


def _check(v, f, shape, tag):
    """one launch of the lattice kernel == the existing kernel == the numpy restatement"""
    d2, idx = ops.distance_field_batch([_mesh(v, f)], shape)
    assert d2.shape == idx.shape == (1,) + tuple(shape) and d2.dtype == torch.float64 and idx.dtype == torch.int32, tag
    pd2, pidx = _at_lattice_points(v, f, shape)
    assert torch.equal(idx[0], pidx) and torch.equal(d2[0], pd2), tag
    rd2, ridx = DF.distance_field_reference(v, f, shape)
    assert np.array_equal(idx[0].cpu().numpy(), ridx) and np.array_equal(d2[0].cpu().numpy(), rd2), tag
    return d2[0], idx[0]


@pytest.fixture(scope="module")
def meshes():
    rng = np.random.default_rng(0)
    v, f = sheet(12, rng, z=0.4, amp=0.2)
    big_v, big_f = sheet(32, rng, z=0.55, amp=0.15)
    assert len(f) == 242 and len(big_f) == 1922
    return dict(v=v, f=f, big_v=big_v, big_f=big_f)


# ------------------------------------------------------------------------------------------------ equal to the existing kernel and to numpy
@pytest.mark.parametrize("shape", LATTICES)
@pytest.mark.parametrize("nf", FACE_COUNTS)
def test_field_is_the_existing_kernel_at_the_lattice_points(meshes, nf, shape):
    d2, idx = _check(meshes["v"], meshes["f"][:nf], shape, f"F={nf} {shape}")
    assert torch.isfinite(d2).all() and int(idx.min()) >= 0 and int(idx.max()) < nf


def test_many_tiles_and_many_spans(meshes):
    d2, idx = _check(meshes["big_v"], meshes["big_f"], (17, 17, 17), "F=1922 17^3")
    assert len(torch.unique(idx)) > 100                                  # the minimum really moves across the tiles
    via_module = DF.distance_field([(meshes["big_v"], meshes["big_f"])], (17, 17, 17))
    assert np.array_equal(via_module[0][0], d2.cpu().numpy()) and np.array_equal(via_module[1][0], idx.cpu().numpy())


# ------------------------------------------------------------------------------------------------ batches
def test_ragged_batch_with_an_empty_mesh(meshes):
    shape = (5, 6, 7)
    batch = [(meshes["v"], meshes["f"][:1]), (np.zeros((0, 3)), np.zeros((0, 3), np.int32)), (meshes["v"], meshes["f"])]
    d2, idx = ops.distance_field_batch([_mesh(v, f) for v, f in batch], shape)
    assert d2.shape == idx.shape == (3,) + shape
    assert torch.isposinf(d2[1]).all() and bool((idx[1] == -1).all())
    for k, (v, f) in enumerate(batch):
        one_d2, one_idx = ops.distance_field_batch([_mesh(v, f)], shape)
        assert torch.equal(d2[k], one_d2[0]) and torch.equal(idx[k], one_idx[0]), k
    again_d2, again_idx = ops.distance_field_batch([_mesh(v, f) for v, f in batch], shape)
    assert torch.equal(d2.view(torch.int64), again_d2.view(torch.int64)) and torch.equal(idx, again_idx)
    assert int(idx[0].max()) == 0 and int(idx[2].max()) > 0


# ------------------------------------------------------------------------------------------------ edge cases
def test_ties_on_a_duplicated_face_and_on_a_shared_vertex():
    # a fan of four faces around the vertex (0.25, 0.5, 0.75) = node (1, 2, 3) of a (5, 5, 5) lattice, its first face repeated
    v = np.array([[0.25, 0.5, 0.75], [0.6, 0.45, 0.8], [0.3, 0.9, 0.7], [-0.1, 0.55, 0.65], [0.2, 0.1, 0.85]])
    fan = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], dtype=np.int32)
    f = np.concatenate([fan[2:3], fan])                                  # face 0 and face 3 are the same triangle
    d2, idx = _check(v, f, (5, 5, 5), "fan")
    assert float(d2[1, 2, 3]) == 0.0 and int(idx[1, 2, 3]) == 0
    assert not bool((idx == 3).any()) and bool((idx == 0).any())         # the copy with the higher index never wins


def test_zero_area_faces(meshes):
    v, f = meshes["v"], meshes["f"][:200].copy()
    f[10:20, 1] = f[10:20, 0]                                            # (v0, v0, v2)
    f[40:45, 2] = f[40:45, 1]                                            # (v0, v1, v1)
    f[50] = f[50, 0]                                                     # a point
    d2, _ = _check(v, f, (5, 6, 7), "zero-area faces")
    assert torch.isfinite(d2).all()
    d2, _ = _check(v, f[[50, 12, 41]], (5, 6, 7), "only zero-area faces")
    assert torch.isfinite(d2).all() and float(d2.min()) > 0


def test_bad_face_index_raises_and_leaves_the_next_call_alone(meshes):
    mesh = _mesh(meshes["v"], meshes["f"][:200])
    before = ops.distance_field_batch([mesh], (5, 5, 5))
    bad = meshes["f"][:200].copy()
    bad[150, 1] = len(meshes["v"])
    with pytest.raises(IndexError):
        ops.distance_field_batch([(_d(meshes["v"]), _d(bad, torch.int32))], (5, 5, 5))
    bad[150, 1] = -1
    with pytest.raises(IndexError):
        ops.distance_field_batch([mesh, (_d(meshes["v"]), _d(bad.astype(np.int64) + 2 ** 33, torch.int64))], (5, 5, 5))
    after = ops.distance_field_batch([mesh], (5, 5, 5))
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_limits_are_refused_by_name(meshes):
    mesh = _mesh(meshes["v"], meshes["f"][:4])
    for shape in ((1, 5, 5), (5, 5, 1), (2048, 1024, 1024)):
        with pytest.raises(ValueError, match="gn_distance_field_batch"):
            ops.distance_field_batch([mesh], shape)
    with pytest.raises(ValueError):
        ops.distance_field_batch([], (5, 5, 5))
    with pytest.raises(TypeError):
        ops.distance_field_batch([(mesh[0], mesh[1].double())], (5, 5, 5))
    with pytest.raises(ValueError):
        ops.distance_field_batch([(mesh[0][:, :2], mesh[1])], (5, 5, 5))


# ------------------------------------------------------------------------------------------------ prepare, both backends
def test_prepare_builds_the_same_bits_with_both_backends_and_feeds_the_training_loop(tmp_path):
    size = 9
    store = str(tmp_path / "hip.zarr")
    keys = write_mesh_store(store, [open_box_mesh(s, drop=s) for s in range(3)])
    args = ["--volume_size", str(size), "--batch_size", "2"]
    P.main(["--zarr_in", store, "--backend", "numpy", "--groups", "nocs_winding_number_field"] + args)
    other = str(tmp_path / "numpy.zarr")
    shutil.copytree(store, other)
    for path, backend in ((store, "hip"), (other, "numpy")):
        summary = P.main(["--zarr_in", path, "--backend", backend, "--groups", "--derived_groups"] + list(P.DERIVED_GROUPS) + args)
        assert summary["written"] == {g: 3 for g in P.DERIVED_GROUPS}
    a, b = (zarr_store.open_group(p, create=False)["samples"] for p in (store, other))
    for key in keys:
        for g in P.DERIVED_GROUPS:
            x, y = a[key]["volume"][g][str(size)][:], b[key]["volume"][g][str(size)][:]
            assert x.dtype == np.float32 and x.shape == (size,) * 3 and np.array_equal(x.view(np.int32), y.view(np.int32)), (key, g)
        signed = a[key]["volume"]["nocs_signed_distance_field"][str(size)][:]
        assert signed[4, 4, 4] < 0 < signed[0, 0, 0]
    # the store now feeds the training loop with the matching volume_group: resident batches are the host dataset's, a step runs on them
    for group, kw, hp in (("nocs_signed_distance_field", dict(tsdf_clip_value=0.05), dict()),
                          ("nocs_occupancy_grid", dict(), dict(volume_classification=True))):
        ds = GarmentInputDataset(store, num_pc_sample=200, volume_size=size, num_volume_sample=96, num_surface_sample=80, static_epoch_seed=True,
                                 enable_augumentation=False, volume_group=group, **kw)
        chunk = [2, 0, 1]
        host = GarmentInputDataset.collate([ds[k] for k in chunk])
        got = ResidentDataset(ds, [0, 1, 2], DEV).batch(chunk)
        for k in ("volume_query_points", "gt_volume_value", "surf_query_points", "gt_sim_points"):
            assert torch.equal(getattr(got, k).cpu(), getattr(host, k)), (group, k)
        values = got.gt_volume_value
        assert bool(torch.isfinite(values).all()) and float(values.min()) < float(values.max())
        assert float(values.abs().max()) <= 1.0 + 8 * 2.0 ** -23         # clipped to [-1, 1], then eight fp32 trilinear weights that sum to 1
        if group == "nocs_occupancy_grid":
            assert set(values.unique().tolist()) == {0.0, 1.0}
        model = small_model(1, planted_nocs=True, reduce_method="max", **hp).to(DEV).requires_grad_(True).train()
        metrics = TP.train_step(model, model.configure_optimizers(), got)
        assert {"loss", "volume_loss", "surface_loss"} <= set(metrics) and all(math.isfinite(v) for v in metrics.values()), (group, metrics)
