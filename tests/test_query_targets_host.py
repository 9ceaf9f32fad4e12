"""CPU: the numpy restatement of the exact volume targets (garmentnets_amd/targets.py), the resident layout without a volume and the --exact_targets flag.

The bounds are the project's own: the closed box holds |w - 1| <= 6.7e-16 inside and |w| <= 1.4e-16 outside (tests/test_winding_host.py); a sum of F solid
angles in another order stays within F * 2**-50 of winding_number_reference.  Why (DESIGN.md "Exact volume targets" has it in full): both orders add the
SAME F terms, so they differ by their additions' roundings alone; an addition errs by at most 2**-53 of its result, every result is a partial sum of solid
angles of a sub-surface, at most 8 pi in magnitude (|partial w| <= 2) for a garment-like sheet, and each order has at most F additions that round: at most
2 * F * 2**-53 * 8 pi / (4 pi) = F * 2**-51, plus the two divisions' 2 * 2**-53 * |w|.  Everything else is bit equality.
"""
import numpy as np
import pytest

from garmentnets_amd import distance as DI
from garmentnets_amd import targets as TG
from garmentnets_amd import train as T
from garmentnets_amd import train_pipeline as TP
from garmentnets_amd import winding as W
from garmentnets_amd.io import resident as R
from test_resident_host import COUNTS
from test_winding_host import BOX_HI, BOX_LO, box_mesh, open_box_mesh

DERIVED = (DI.DISTANCE_GROUP, DI.SIGNED_DISTANCE_GROUP, DI.OCCUPANCY_GROUP)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _lattice32(shape):
    pts = W.lattice_points(shape)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)          # i / 4 and i / 8: exact in fp32 and fp64
    return pts.astype(np.float32)


@pytest.fixture(scope="module")
def garment():
    v, f = open_box_mesh(3)
    assert v.dtype == np.float32 and 30 <= len(f) <= TG.QT_FACE_CHUNK
    return v, f


def test_the_chunk_is_the_librarys_constant():
    assert TG.QT_FACE_CHUNK == TG.face_chunk() >= 1 and isinstance(TG.QT_FACE_CHUNK, int)
    assert set(TG.KINDS) == set(__import__("garmentnets_amd")._lib.QT_KINDS)


def test_closed_box_inside_and_outside():
    v64, f = box_mesh()
    v = v64.astype(np.float32)
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    q = _lattice32((9, 9, 9))
    inside = np.all((q > lo) & (q < hi), axis=1)
    assert 0 < inside.sum() < len(q) and np.array_equal(inside, np.all((q > np.asarray(BOX_LO)) & (q < np.asarray(BOX_HI)), axis=1))
    dist, _, d2, _ = TG.query_targets_reference(q, v, f, DI.DISTANCE_GROUP)
    signed, w, d2s, _ = TG.query_targets_reference(q, v, f, DI.SIGNED_DISTANCE_GROUP)
    occ, w_o, none_d2, none_idx = TG.query_targets_reference(q, v, f, DI.OCCUPANCY_GROUP)
    assert none_d2 is None and none_idx is None and np.array_equal(_bits(w), _bits(w_o)) and np.array_equal(_bits(d2), _bits(d2s))
    err_in, err_out = np.abs(w[inside] - 1).max(), np.abs(w[~inside]).max()
    print(f"[query targets] closed box on 9^3: |w - 1| inside {err_in:.2e}, |w| outside {err_out:.2e}")
    assert err_in <= 6.7e-16 and err_out <= 1.4e-16
    assert np.array_equal(occ, inside.astype(np.float32))
    assert dist.dtype == np.float32 and (dist > 0).all()
    assert np.array_equal(_bits(signed[inside]), _bits(-dist[inside])) and np.array_equal(_bits(signed[~inside]), _bits(dist[~inside]))


def test_lattice_nodes_are_the_prepared_volumes(garment):
    v, f = garment
    shape = (5, 5, 5)
    q = _lattice32(shape)
    w32 = W.winding_field_reference(v, f, shape)
    for group in TG.WINDING_GROUPS:
        got = TG.query_targets_reference(q, v, f, group)[0]
        assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(w32.reshape(-1))), group
    d2, idx = DI.distance_field_reference(v, f, shape)
    for group in DERIVED:
        got, _, got_d2, got_idx = TG.query_targets_reference(q, v, f, group)
        assert np.array_equal(_bits(got), _bits(DI.derived_volume(group, d2, w32).reshape(-1))), group
        if group != DI.OCCUPANCY_GROUP:
            assert np.array_equal(_bits(got_d2), _bits(d2.reshape(-1))) and np.array_equal(got_idx, idx.reshape(-1))


def test_chunk_order(garment):
    v, f = garment
    f = f[:30]
    q = np.random.default_rng(2).random((200, 3)).astype(np.float32)
    want = W.winding_number_reference(q.astype(np.float64), v, f)
    assert np.abs(want).max() > 0.1
    for chunk in (30, 31, 512, None):                                         # chunk >= F: the reference's bits
        assert np.array_equal(_bits(TG.query_targets_reference(q, v, f, "nocs_winding_number_field", chunk=chunk)[1]), _bits(want)), chunk
    for chunk in (1, 7):
        got = TG.query_targets_reference(q, v, f, "nocs_winding_number_field", chunk=chunk)[1]
        err = float(np.abs(got - want).max())
        print(f"[query targets] chunk {chunk} on 30 faces: max |w - w_ref| {err:.2e}, bound {30 * 2.0 ** -50:.2e}")
        assert err <= 30 * 2.0 ** -50
        # the distance does not see the chunks
        a, b = TG.query_targets_reference(q, v, f, DI.DISTANCE_GROUP, chunk=chunk), TG.query_targets_reference(q, v, f, DI.DISTANCE_GROUP)
        assert np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(a[3], b[3])
    with pytest.raises(ValueError):
        TG.query_targets_reference(q, v, f, "nocs_winding_number_field", chunk=0)


@pytest.mark.parametrize("group", TG.KINDS)
def test_tsdf_clip_and_absolute_are_data_ios_expressions(garment, group):
    v, f = garment
    q = (np.random.default_rng(4).random((300, 3)) * 1.2 - 0.1).astype(np.float32)
    plain = TG.query_targets_reference(q, v, f, group)[0]
    assert plain.dtype == np.float32
    clipped = TG.query_targets_reference(q, v, f, group, tsdf_clip_value=0.05)[0]
    assert np.array_equal(_bits(clipped), _bits(np.clip(plain / 0.05, -1, 1))) and clipped.dtype == np.float32
    assert np.array_equal(_bits(TG.query_targets_reference(q, v, f, group, absolute=True)[0]), _bits(np.abs(plain)))
    both = TG.query_targets_reference(q, v, f, group, tsdf_clip_value=0.3, absolute=True)[0]
    assert np.array_equal(_bits(both), _bits(np.abs(np.clip(plain / 0.3, -1, 1))))
    if group == DI.SIGNED_DISTANCE_GROUP:
        assert (clipped == 1).any() and (clipped == -1).any() and (np.abs(clipped) < 1).any()


def test_empty_mesh_nan_query_and_refusals(garment):
    v, f = garment
    q = np.array([[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5]], dtype=np.float32)
    empty = np.zeros((0, 3), dtype=np.int32)
    t, w, d2, idx = TG.query_targets_reference(q[:1], v, empty, DI.SIGNED_DISTANCE_GROUP)
    assert w[0] == 0 and d2[0] == np.inf and idx[0] == -1 and t[0] == np.inf
    for group in TG.KINDS:
        t = TG.query_targets_reference(q, v, f, group)[0]
        assert np.isfinite(t[0])
        assert t[1] == 0 if group == DI.OCCUPANCY_GROUP else np.isnan(t[1]), group
    with pytest.raises(ValueError, match="marching_cube_mesh"):
        TG.query_targets_reference(q, v, f, "marching_cube_mesh")
    with pytest.raises(TypeError):
        TG.query_targets_reference(q.astype(np.float64), v, f, DI.DISTANCE_GROUP)
    with pytest.raises(IndexError):
        TG.query_targets_reference(q, v[:3], f, DI.DISTANCE_GROUP)


def test_layout_without_a_volume():
    kw = dict(num_volume_sample=10, num_surface_sample=10, num_mc_surface_sample=5, surface_sample_ratio=0.5)
    with_volume, exact = R.held_arrays(**kw), R.held_arrays(**kw, exact_targets=True)
    assert "volume" in with_volume and "volume" not in exact and set(with_volume) - set(exact) == {"volume"}
    voxels = sum(c["voxels"] for c in COUNTS)
    assert R.plan(COUNTS, with_volume).nbytes - R.plan(COUNTS, exact).nbytes == voxels * 4 > 0
    # the task-space field is the one of the task-space vertices: held without the surface sampler too
    assert set(R.held_arrays(num_volume_sample=5, volume_task_space=True, exact_targets=True)) == set(R.held_arrays()) | {"task_verts"}
    assert set(R.held_arrays(num_volume_sample=5, num_surface_sample=5, volume_task_space=True, exact_targets=True)) == \
        set(R.held_arrays()) | {"task_verts", "cdf_task"}
    assert R.held_arrays(num_surface_sample=5, exact_targets=True) == R.held_arrays(num_surface_sample=5)      # no volume queries: the flag changes nothing
    assert R.held_arrays(**kw, exact_targets=False) == with_volume


@pytest.mark.parametrize("mod", [T, TP])
def test_exact_targets_alone_is_an_argparse_error(mod, capsys):
    with pytest.raises(SystemExit) as e:
        mod.parse_args(["--zarr_in", "x.zarr", "--exact_targets"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--exact_targets requires --resident" in err and "usage:" in err
    a = mod.parse_args(["--zarr_in", "x.zarr", "--exact_targets", "--resident"] + (["--model", "pointnet2"] if mod is T else []))
    assert a.exact_targets is True and a.resident is True
