"""CPU: the host side of the resident dataset (garmentnets_amd/io/resident.py) -- the draw functions of io/dataset.py against what the samplers consumed
before they were expressed through them, the CSR / byte arithmetic of the resident layout from shapes alone, the draw buffer's sections, and the new
command-line flags of the two training loops."""
import numpy as np
import pytest

from garmentnets_amd import train as T
from garmentnets_amd import train_loop as L
from garmentnets_amd import train_pipeline as TP
from garmentnets_amd import validate as V
from garmentnets_amd._lib import RESIDENT_META
from garmentnets_amd.common.metrics import barycentric_interpolation, mesh_sample_barycentric
from garmentnets_amd.io import dataset as D
from garmentnets_amd.io import resident as R
from test_validate_host import CASES, case_inputs, gold  # noqa: F401  (gold: the module fixture of the golden validation cases)


def awkward_mesh(seed=0):
    """60 vertices, 200 faces: a block of repeated faces, a block of zero-area ones (a vertex named twice), the rest random"""
    rng = np.random.default_rng(seed)
    verts = rng.random((60, 3)).astype(np.float32)
    faces = rng.integers(0, 60, (200, 3)).astype(np.int32)
    faces[20:40] = faces[7]
    faces[90:110, 1] = faces[90:110, 0]
    return verts, faces


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("seed", [0, 7, None])
def test_mesh_draws_and_sample_faces_are_mesh_sample_barycentric(seed):
    verts, faces = awkward_mesh()
    n = 4096
    bc_ref, face_ref = mesh_sample_barycentric(verts, faces, n, seed=seed)
    face_u, uv = D.SeededDraws(3, False).mesh_draws(n) if seed is None else D.SeededDraws(seed, True).mesh_draws(n)
    assert face_u.shape == (n,) and uv.shape == (n, 2) and face_u.dtype == uv.dtype == np.float64
    bc, face_idx = D.sample_faces(D.face_cdf(verts, faces), face_u, uv, index_dtype=faces.dtype)
    assert face_idx.dtype == face_ref.dtype and bc.dtype == bc_ref.dtype
    if seed is None:                                                  # OS entropy: the contract is the distribution's support, not the values
        assert face_idx.min() >= 0 and face_idx.max() < len(faces) and np.all(bc >= 0) and np.all(bc.sum(1) <= 1 + 1e-15)
        return
    np.testing.assert_array_equal(face_idx, face_ref)
    np.testing.assert_array_equal(bc, bc_ref)
    assert not np.isin(face_idx, np.arange(90, 110)).any()            # a zero-area face is never drawn


def test_face_cdf_is_what_choice_searches_and_refuses_a_mesh_without_area():
    verts, faces = awkward_mesh(1)
    from garmentnets_amd.common.metrics import doublearea
    w = doublearea(verts, faces)
    w = w / np.sum(w)
    u = np.random.RandomState(5).random_sample(2000)
    np.testing.assert_array_equal(np.searchsorted(D.face_cdf(verts, faces), u, side="right"), np.random.RandomState(5).choice(len(faces), 2000, replace=True, p=w))
    with pytest.raises(ValueError):
        with np.errstate(invalid="ignore"):
            D.face_cdf(verts, np.array([[1, 1, 2], [3, 3, 3]]))


@pytest.mark.parametrize("ratio", [0, 0.25, 0.5])
def test_volume_draws_are_the_streams_get_volume_sample_read(ratio):
    """the parent's get_volume_sample, restated: uniform points, then (another fresh stream) the mesh sample, then the noise from the first stream"""
    idx, n, std = 11, 301, 0.07
    rs = np.random.RandomState(idx)
    d = D.SeededDraws(idx, True).volume_draws(n, ratio, std)
    if ratio == 0:
        np.testing.assert_array_equal(d["uniform"], rs.uniform(low=0, high=1, size=(n, 3)).astype(np.float32))
        assert set(d) == {"uniform"}
        return
    n_uniform = int(n * ratio)
    np.testing.assert_array_equal(d["uniform"], rs.uniform(low=0, high=1, size=(n_uniform, 3)).astype(np.float32))
    np.testing.assert_array_equal(d["noise"], rs.normal(loc=(0,) * 3, scale=(std,) * 3, size=(n - n_uniform, 3)))
    rs2 = np.random.RandomState(idx)
    np.testing.assert_array_equal(d["face_u"], rs2.random_sample(n - n_uniform))
    np.testing.assert_array_equal(d["uv"], rs2.uniform(0, 1, size=(n - n_uniform, 2)))
    assert d["uniform"].dtype == np.float32 and d["noise"].dtype == d["face_u"].dtype == d["uv"].dtype == np.float64


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_reexpressed_samplers_equal_the_parent_on_the_golden_store(gold, ci):  # noqa: F811
    """the three samplers through the draw functions against their parent's formulation (mesh_sample_barycentric on a seed) and the reference's values"""
    (idx, ratio, group, clip, absval, _, _, mc, nvol, nsurf), data_in, grp = case_inputs(gold, ci)
    volume = D.read_volume(grp, group, 9, clip, absval)
    task = group == D.TASK_SPACE_VOLUME_GROUP
    got = D.get_surface_sample(idx, data_in, nsurf, True, task, gold[f"d{ci}/aabb"])
    qv, tv = data_in["cloth_nocs_verts"], data_in["cloth_sim_verts"]
    if task:
        qv, tv = D.AABBGripNormalizer(gold[f"d{ci}/aabb"])(tv), qv
    bc, fi = mesh_sample_barycentric(qv, data_in["cloth_faces_tri"], nsurf, seed=idx)
    np.testing.assert_array_equal(got["surf_query_points"][0], barycentric_interpolation(bc, qv, data_in["cloth_faces_tri"][fi]))
    np.testing.assert_array_equal(got["gt_sim_points"][0], barycentric_interpolation(bc, tv, data_in["cloth_faces_tri"][fi]))
    np.testing.assert_array_equal(got["surf_query_points"], gold[f"d{ci}/surf/surf_query_points"])
    vol = D.get_volume_sample(idx, data_in, volume, nvol, ratio, 0.05, True, group)
    np.testing.assert_array_equal(vol["volume_query_points"], gold[f"d{ci}/vol/volume_query_points"])
    if mc:
        m = D.get_mc_surface_sample(idx, data_in, nsurf, True)
        np.testing.assert_array_equal(m["mc_surf_query_points"], gold[f"d{ci}/mc/mc_surf_query_points"])
        np.testing.assert_array_equal(m["is_query_point_on_surf"], gold[f"d{ci}/mc/is_query_point_on_surf"])


def test_rotation_angle_draw_is_the_matrix_draw():
    from scipy.spatial.transform import Rotation
    dr = D.SeededDraws(4, True)
    np.testing.assert_array_equal(dr.z_rotation(-90, 90), Rotation.from_euler("z", dr.z_angle(-90, 90), degrees=True).as_matrix().astype(np.float32))
    assert dr.z_angle(-90, 90) == np.random.RandomState(4).uniform(-90, 90)


# ------------------------------------------------------------------------------------------------ layout
COUNTS = [dict(points=768, verts=40, faces=70, mc_verts=50, mc_faces=80, voxels=125),
          dict(points=900, verts=3, faces=1, mc_verts=20, mc_faces=1, voxels=125),
          dict(points=0, verts=25, faces=30, mc_verts=35, mc_faces=60, voxels=125)]


def test_plan_csr_tables_and_nbytes_from_shapes_alone():
    names = R.held_arrays(num_volume_sample=10, num_surface_sample=10, num_mc_surface_sample=5, surface_sample_ratio=0.5)
    assert set(names) == {"pc_sim", "pc_nocs", "pc_rgb", "sim_verts", "nocs_verts", "faces", "cdf_nocs", "mc_verts", "mc_flags", "mc_faces", "cdf_mc", "volume"}
    lay = R.plan(COUNTS, names)
    np.testing.assert_array_equal(lay.offsets["points"], [0, 768, 1668, 1668])
    np.testing.assert_array_equal(lay.offsets["faces"], [0, 70, 71, 101])
    np.testing.assert_array_equal(lay.offsets["mc_faces"], [0, 80, 81, 141])
    assert all(v.dtype == np.int64 and len(v) == len(COUNTS) + 1 for v in lay.offsets.values())
    assert lay.arrays["pc_rgb"] == (1668, 3, np.dtype(np.uint8)) and lay.arrays["cdf_nocs"] == (101, 1, np.dtype(np.float64))
    pts, verts, faces, mcv, mcf, vox = 1668, 68, 101, 105, 141, 375
    want = pts * (12 + 12 + 3) + verts * 24 + faces * (12 + 8) + mcv * (12 + 4) + mcf * (12 + 8) + vox * 4 + 3 * len(RESIDENT_META) * 8 + 3 * 24 + 24
    assert lay.nbytes == want
    # the staging buffer: the largest sample, every array padded to 8 bytes
    s0 = [768 * 12, 768 * 12, 768 * 3, 40 * 12, 40 * 12, 70 * 12, 70 * 8, 50 * 12, 50 * 4, 80 * 12, 80 * 8, 125 * 4]
    s1 = [900 * 12, 900 * 12, 900 * 3, 36, 36, 12, 8, 240, 80, 12, 8, 500]
    assert lay.staging_bytes == max(sum((b + 7) // 8 * 8 for b in s) for s in (s0, s1))


def test_held_arrays_follow_the_sampler_settings():
    base = {"pc_sim", "pc_nocs", "pc_rgb", "sim_verts", "nocs_verts", "faces"}
    assert set(R.held_arrays()) == base
    assert set(R.held_arrays(num_volume_sample=5)) == base | {"volume"}                                        # uniform queries: no mesh table
    assert set(R.held_arrays(num_surface_sample=5, volume_task_space=True)) == base | {"task_verts", "cdf_task"}
    assert set(R.held_arrays(num_volume_sample=5, surface_sample_ratio=0.5, num_surface_sample=5, volume_task_space=True)) == \
        base | {"volume", "cdf_nocs", "task_verts", "cdf_task"}
    lay = R.plan(COUNTS, R.held_arrays())
    assert lay.nbytes == 1668 * 27 + 68 * 24 + 101 * 12 + 3 * len(RESIDENT_META) * 8 + 3 * 24 + 24


def test_plan_offsets_stay_int64_past_2_31_elements():
    big = [dict(points=1, verts=3, faces=1, mc_verts=0, mc_faces=0, voxels=128 ** 3)] * 1100
    lay = R.plan(big, R.held_arrays(num_volume_sample=1))
    assert lay.offsets["voxels"][-1] == 1100 * 128 ** 3 > 2 ** 31 and lay.nbytes > 1100 * 128 ** 3 * 4


def test_draw_sections_are_aligned_disjoint_and_sized():
    lay = R.draw_sections(3, 333, num_volume_sample=257, n_uniform=128, num_surface_sample=131, mc=True, near=True, pc_noise=True, rotation=True)
    assert set(lay.sections) == {"vol_face_u", "vol_uv", "vol_noise", "surf_face_u", "surf_uv", "mc_face_u", "mc_uv", "pc_noise", "vol_uniform", "rot", "sel",
                                 "slots"}
    end = 0
    for name, (off, dt, shape) in lay.sections.items():
        assert off == end and off % dt.itemsize == 0, name
        end = off + int(np.prod(shape)) * dt.itemsize
    assert end <= lay.nbytes < end + 8 and lay.nbytes % 8 == 0
    assert lay.sections["vol_noise"][2] == (3, 129, 3) and lay.sections["sel"][1] == np.int32
    plain = R.draw_sections(1, 50)
    assert list(plain.sections) == ["sel", "slots"] and plain.nbytes == 208


# ------------------------------------------------------------------------------------------------ command line
@pytest.mark.parametrize("mod", [T, TP])
def test_new_flags_default_off(mod):
    a = mod.build_parser().parse_args(["--zarr_in", "x"])
    assert (a.resident, a.resident_gib, a.shuffle) == (False, None, False)
    b = mod.build_parser().parse_args(["--zarr_in", "x", "--resident", "--resident_gib", "1.5", "--shuffle"])
    assert (b.resident, b.resident_gib, b.shuffle) == (True, 1.5, True)


def test_shuffle_order_depends_on_seed_and_epoch_only():
    idx = np.arange(100, 140)
    assert L.epoch_order(idx, False, 0, 3) is not None and np.array_equal(L.epoch_order(idx, False, 0, 3), idx)
    a = L.epoch_order(idx, True, 2, 1)
    assert np.array_equal(a, L.epoch_order(idx, True, 2, 1)) and np.array_equal(np.sort(a), idx)
    assert np.array_equal(a, idx[np.random.RandomState(3).permutation(len(idx))])
    assert not np.array_equal(a, L.epoch_order(idx, True, 2, 2)) and not np.array_equal(a, L.epoch_order(idx, True, 5, 1))
    assert np.array_equal(a, L.epoch_order(idx, True, 1, 2))                                # RandomState(seed + epoch), as stated


def test_validation_rows_takes_another_batch_source():
    class Model:
        def validation_metrics(self, batch):
            return {"loss": float(batch.v)}

    class B:
        def __init__(self, v):
            self.v = v

        def to(self, device):
            return self
    rows = V.validation_rows(Model(), None, None, 2, None, "cpu", batches=iter([([0, 1], B(1.0)), ([2], B(4.0))]))
    assert [(r["garments"], r["val_loss"]) for r in rows] == [(2, 1.0), (1, 4.0)] and V.epoch_values(rows) == {"val_loss": 2.0}
