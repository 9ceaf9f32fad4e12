"""Host side of the point clouds from meshes (no GPU): the numpy restatement of garmentnets_amd/point_cloud.py against what the definitions of
DESIGN.md "Point clouds from meshes" must give, and `python -m garmentnets_amd.prepare --point_clouds --backend numpy` on a store that holds meshes
and nothing else.  tests/test_gpu_point_cloud.py holds the device to this restatement bit for bit.

The bounds:
  reprojection  1/512 + 1e-3 px per axis.  The weights are exact barycentrics of the SNAPPED screen triangle and perspective-correct mixing maps them
                linearly onto the true one, so a point misses its sample by at most the largest vertex snap, half a fixed-point step (1/512 px); the
                1e-3 covers the fp32 rounding of the stored point.  Measured here: 0.0016 .. 0.0019 px.
  labels        2e-7 absolute: the fp32 rounding of two outputs of magnitude below 1 (measured 6e-8).  Labels mixed screen-linearly from the same
                weights miss by a thousand times the bound and more, which the same test asserts: it would catch that mistake.

The mesh-only store builder and the hand-made cameras below are shared with tests/test_gpu_point_cloud.py.
"""
import numpy as np
import pytest

from garmentnets_amd import point_cloud as PC
from garmentnets_amd import prepare as P
from garmentnets_amd.io import zarr_store
from garmentnets_amd.io.dataset import GarmentInputDataset, data_io, get_base_data
from test_winding_host import AABB, open_box_mesh

NONE = 0xFFFFFFFF
SIM_SCALE, SIM_SHIFT = np.float32([0.7, 0.7, 0.9]), np.float32([0.0, 0.0, -0.43])
REPROJECTION_BOUND = 1.0 / 512 + 1e-3
LABEL_BOUND = 2e-7


def to_sim(nocs):
    """write_mesh_store's affine map of the NOCS cube into the store's bounding box, in fp32"""
    return ((np.asarray(nocs, np.float32) - np.float32(0.5)) * SIM_SCALE + SIM_SHIFT).astype(np.float32)


def garment(seed, n=2, drop=0):
    """(sim verts, NOCS verts, faces) of an open box"""
    nocs, faces = open_box_mesh(seed, n=n, drop=drop)
    return to_sim(nocs), nocs, faces


def pinhole(S, f=None, near=0.1):
    """the camera at the origin looking along +z: world coordinates are camera coordinates"""
    return {"R": np.eye(3), "t": np.zeros(3), "f": float(S / 2 if f is None else f), "c": S / 2, "near": near}


def project(points, cam):
    p = PC.to_camera(points, cam)
    return cam["f"] * p[:, 0] / p[:, 2] + cam["c"], cam["f"] * p[:, 1] / p[:, 2] + cam["c"]


def cloud(verts, nocs, faces, cam, S, **kw):
    """(index image, point, nocs, rgb) of one view through the restatement"""
    idx = PC.render_depth_idx_numpy(verts, faces, cam, S)
    return (idx,) + PC.depth_cloud_numpy(idx, verts, nocs, faces, cam, **kw)


def square(x0, x1, y0, y1, z):
    """two triangles sharing the diagonal 0 - 2"""
    v = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def write_mesh_only_store(path, meshes):
    """a dataset store with mesh/*, the attributes and summary/cloth_aabb_union, and NO point_cloud.  meshes: [(sim verts, NOCS verts, faces)]"""
    root = zarr_store.open_group(str(path))
    root.require_group("summary").array("cloth_aabb_union", AABB)
    keys = []
    for i, (sim, nocs, faces) in enumerate(meshes):
        key = f"{i:05d}_Dress_{i:06d}_0"
        keys.append(key)
        sg = root.require_group("samples").require_group(key)
        sg.put_attrs({"scale": 1.0 + 0.1 * i, "sample_id": f"{i:05d}_Dress", "garment_name": "Dress", "grip_vertex_idx": i % len(nocs)})
        mesh = sg.require_group("mesh")
        mesh.array("cloth_verts", np.asarray(sim, dtype=np.float32))
        mesh.array("cloth_nocs_verts", np.asarray(nocs, dtype=np.float32))
        mesh.array("cloth_faces_tri", np.asarray(faces, dtype=np.int32))
    return keys


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def box_views():
    """S -> [(camera, index image, point, nocs, rgb)] of the four ring views of one open box, rendered once"""
    sim, nocs, faces = garment(0, n=3)
    return {S: [(cam,) + cloud(sim, nocs, faces, cam, S) for cam in PC.camera_ring(AABB, 4, S)] for S in (32, 40)}, (sim, nocs, faces)


@pytest.mark.parametrize("S", [32, 40])
def test_every_point_projects_back_into_its_own_sample(box_views, S):
    worst = 0.0
    for cam, idx, point, _, _ in box_views[0][S]:
        Y, X = np.nonzero(idx != NONE)
        assert len(point) == len(Y) > 4 * S and point.dtype == np.float32
        u, v = project(point, cam)
        worst = max(worst, float(np.abs(u - (X + 0.5)).max()), float(np.abs(v - (Y + 0.5)).max()))
    print(f"[point_cloud] S={S}: reprojection error {worst:.5f} px (bound {REPROJECTION_BOUND:.5f})")
    assert worst <= REPROJECTION_BOUND


@pytest.mark.parametrize("S", [32, 40])
def test_labels_are_perspective_correct(box_views, S):
    sim, nocs, faces = box_views[1]
    good = wrong = 0.0
    for cam, idx, point, label, _ in box_views[0][S]:
        assert label.dtype == np.float32 and label.shape == point.shape
        good = max(good, float(np.abs(to_sim(label).astype(np.float64) - point).max()))
        lin_label = PC.depth_cloud_numpy(idx, sim, nocs, faces, cam, screen_linear=True)[1]      # the same w_k, mixed as w_k / area2
        wrong = max(wrong, float(np.abs(to_sim(lin_label).astype(np.float64) - point).max()))
    print(f"[point_cloud] S={S}: |affine(nocs) - point| {good:.2e} (bound {LABEL_BOUND:.0e}); with screen-linear labels {wrong:.2e}")
    assert good <= LABEL_BOUND
    assert wrong > 1000 * LABEL_BOUND                                    # orders of magnitude: this test would catch screen-linear mixing


def test_the_label_of_a_point_is_the_label_of_its_place_on_the_face():
    """one slanted face with a NOCS map that is NOT affine in the screen: the label at a pixel is the label of the 3-D point the pixel's ray hits"""
    S, cam = 32, pinhole(32)
    verts = np.array([[-0.9, -0.8, 1.0], [2.5, -0.5, 4.0], [-0.5, 2.0, 3.0]], dtype=np.float32)
    nocs = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0, 0.25]], dtype=np.float32)
    idx, point, label, _ = cloud(verts, nocs, [[0, 1, 2]], cam, S)
    assert len(point) > 100
    # solve for each point's barycentrics in the 3-D triangle, from the point alone, and mix the labels with them
    T = np.stack([verts[1] - verts[0], verts[2] - verts[0]], axis=1).astype(np.float64)
    st = np.linalg.lstsq(T, (point.astype(np.float64) - verts[0]).T, rcond=None)[0].T
    assert (st > -1e-6).all() and (st.sum(axis=1) < 1 + 1e-6).all()                       # a convex combination: in the triangle, not merely on the ray
    want = nocs[0] + st[:, :1] * (nocs[1] - nocs[0]) + st[:, 1:] * (nocs[2] - nocs[0])
    assert np.abs(want - label).max() < 1e-6
    lin = PC.depth_cloud_numpy(idx, verts, nocs, [[0, 1, 2]], cam, screen_linear=True)[1]
    assert np.abs(want - lin).max() > 0.05


def test_occlusion_and_equal_depths():
    S, cam = 32, pinhole(32, f=16.0)                                     # u = 16 x / z + 16
    near_v, near_f = square(-0.5, 0.5, -0.5, 0.5, 2.0)                    # u in [12, 20]
    far_v, far_f = square(-3.0, 3.0, -3.0, 3.0, 4.0)                      # u in [4, 28]
    verts, faces = np.concatenate([far_v, near_v]), np.concatenate([far_f, near_f + 4])
    idx, point, _, _ = cloud(verts, verts, faces, cam, S)
    u, v = project(point, cam)
    inside = (u > 12) & (u < 20) & (v > 12) & (v < 20)
    assert inside.sum() == 64 and len(point) == 24 * 24
    assert (point[inside, 2] == 2.0).all() and (point[~inside, 2] == 4.0).all()
    assert set(np.unique(idx[12:20, 12:20])) <= {2, 3} and not np.isin(idx, [2, 3])[:12].any()
    # two coincident faces with different labels: the lower index supplies every point
    tri = np.array([[-1.0, -1.0, 2.0], [1.5, -0.5, 3.0], [-0.5, 1.5, 2.5]], dtype=np.float32)
    verts = np.concatenate([tri, tri])
    nocs = np.concatenate([np.full((3, 3), 0.25, np.float32), np.full((3, 3), 0.75, np.float32)])
    for faces, first in (([[3, 4, 5], [0, 1, 2]], 0.75), ([[0, 1, 2], [3, 4, 5]], 0.25), ([[0, 2, 1], [3, 4, 5]], 0.25)):
        idx, point, label, _ = cloud(verts, nocs, faces, cam, S)
        assert len(point) > 50 and set(np.unique(idx)) == {0, NONE} and (label == np.float32(first)).all()


def test_flipping_every_face_changes_no_bit(box_views):
    """(a, b, c) -> (a, c, b): the swap of b and c restores the very same operand order, so not a bit moves"""
    sim, nocs, faces = box_views[1]
    for cam, idx, point, label, rgb in box_views[0][40]:
        got = cloud(sim, nocs, faces[:, [0, 2, 1]], cam, 40)
        assert np.array_equal(got[0], idx) and np.array_equal(got[1].view(np.uint32), point.view(np.uint32))
        assert np.array_equal(got[2].view(np.uint32), label.view(np.uint32)) and np.array_equal(got[3], rgb)


@pytest.mark.parametrize("turned", [False, True])
def test_a_square_of_two_triangles_yields_one_point_per_covered_sample(turned):
    S, cam = 32, pinhole(32, f=16.0)
    verts, faces = square(-0.9375, 1.0625, -0.6875, 0.8125, 2.0)          # corners ON samples: u = 8.5, 24.5, v = 10.5, 22.5; the diagonal crosses samples
    if turned:
        faces = faces[:, [0, 2, 1]]
    u, v = project(verts, cam)
    assert sorted(set(u)) == [8.5, 24.5] and sorted(set(v)) == [10.5, 22.5]
    # with y down the square owns its right and its bottom edge: the samples in (lo, hi] on each axis
    centres = np.arange(S) + 0.5
    nx, ny = int(((centres > u.min()) & (centres <= u.max())).sum()), int(((centres > v.min()) & (centres <= v.max())).sum())
    idx, point, _, _ = cloud(verts, verts, faces, cam, S)
    assert (nx, ny) == (16, 12) and len(point) == nx * ny
    Y, X = np.nonzero(idx != NONE)
    assert X.min() == 9 and X.max() == 24 and Y.min() == 11 and Y.max() == 22 and set(np.unique(idx)) == {0, 1, NONE}
    pu, pv = project(point, cam)
    assert np.array_equal(pu, X + 0.5) and np.array_equal(pv, Y + 0.5)    # exact here: z is constant and the coordinates are dyadic


def test_guard_faces_contribute_nothing_and_raise_nothing(box_views):
    sim, nocs, faces = box_views[1]
    cam = box_views[0][32][0][0]
    p = PC.to_camera(sim, cam)
    behind = sim[0] + (cam["near"] / 2 - p[0, 2]) * np.asarray(cam["R"])[2]           # vertex 0 moved along the view axis to half the near distance
    assert PC.to_camera(behind[None].astype(np.float32), cam)[0, 2] < cam["near"]
    verts = np.concatenate([sim, [[np.nan, 0.0, 0.0]], [behind], [[np.inf, 0.0, 0.0]]]).astype(np.float32)
    labels = np.concatenate([nocs, np.zeros((3, 3), np.float32)])
    n = len(sim)
    guards = np.array([[0, 1, n + 5], [0, -1, 2], [0, 1, n], [n + 1, 1, 2], [0, n + 2, 2], [3, 3, 4]], dtype=np.int32)
    want = box_views[0][32][0][1:]
    got = cloud(verts, labels, np.concatenate([faces, guards]), cam, 32)
    for g, w in zip(got, want):
        assert np.array_equal(g, w, equal_nan=True)
    alone = cloud(verts, labels, guards, cam, 32)
    assert (alone[0] == NONE).all() and alone[1].shape == (0, 3) and alone[3].shape == (0, 3) and alone[3].dtype == np.uint8


def test_colour_is_a_headlight_shade_of_the_base_colour():
    S, cam = 32, pinhole(32, f=16.0)
    verts, faces = square(-0.5, 0.5, -0.5, 0.5, 2.0)
    _, point, _, rgb = cloud(verts, verts, faces, cam, S, ambient=0.25, base_color=(1.0, 0.5, 0.0))
    # facing the camera: n is along z, so |n.p| / (|n| |p|) = z / |p|
    shade = 0.25 + 0.75 * (2.0 / np.linalg.norm(point.astype(np.float64), axis=1))
    want = np.rint(255 * shade[:, None] * np.array([1.0, 0.5, 0.0]))
    assert rgb.dtype == np.uint8 and np.abs(rgb.astype(np.int64) - want).max() <= 1 and (rgb[:, 2] == 0).all() and rgb[:, 0].max() >= 250
    _, _, _, flat = cloud(verts, verts, faces, cam, S, ambient=1.0, base_color=(2.0, 0.5, -1.0))
    assert (flat == np.array([255, 128, 0], dtype=np.uint8)).all()        # clamped; rint(127.5) = 128, half to even


def test_camera_ring():
    S = 40
    cams = PC.camera_ring(AABB, 5, S, azimuth0=30.0)
    box = AABB.astype(np.float64)
    corners = np.array([[box[i][0], box[j][1], box[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    target, r = box.mean(axis=0), np.linalg.norm(box[1] - box[0]) / 2
    half = np.radians(PC.DEFAULT_FOV) / 2
    for k, cam in enumerate(cams):
        R, t = cam["R"], cam["t"]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
        eye = -R.T @ t
        assert abs(np.linalg.norm(eye - target) - r / np.sin(half)) < 1e-12
        az = np.degrees(np.arctan2(eye[1] - target[1], eye[0] - target[0])) % 360
        assert abs(az - (30.0 + 72.0 * k) % 360) < 1e-9
        assert abs(np.degrees(np.arcsin((eye[2] - target[2]) / np.linalg.norm(eye - target))) - PC.DEFAULT_ELEVATION) < 1e-9
        assert R[1] @ [0, 0, 1] < 0                                       # up = +z: the image's y axis points down
        q = R @ target + t
        assert np.abs(cam["f"] * q[:2] / q[2] + cam["c"] - S / 2).max() < 1e-9 and cam["c"] == S / 2
        pc = corners @ R.T + t
        uv = cam["f"] * pc[:, :2] / pc[:, 2:] + cam["c"]
        assert (pc[:, 2] > cam["near"]).all() and (uv > 0).all() and (uv < S).all()
        assert cam["near"] == pytest.approx((r / np.sin(half) - r) / 2) and cam["f"] == pytest.approx((S / 2) / np.tan(half))
    with pytest.raises(ValueError, match="does not clear the bounding sphere"):
        PC.camera_ring(AABB, 4, S, distance=0.1)
    with pytest.raises(ValueError, match="elevation"):
        PC.camera_ring(AABB, 4, S, elevation=90.0)


def test_render_point_clouds_stacks_the_views_of_every_garment():
    S = 32
    cams = PC.camera_ring(AABB, 3, S)
    meshes = [garment(1), garment(2, n=3, drop=4)]
    out = PC.render_point_clouds(meshes, cams, S, backend="numpy")
    assert len(out) == 2
    for (sim, nocs, faces), o in zip(meshes, out):
        views = [cloud(sim, nocs, faces, cam, S)[1:] for cam in cams]
        assert o["sizes"].dtype == np.int64 and o["sizes"].tolist() == [len(v[0]) for v in views] and o["sizes"].min() > 0
        for k, name in enumerate(("point", "nocs", "rgb")):
            assert np.array_equal(o[name], np.concatenate([v[k] for v in views]))
    assert PC.render_point_clouds([], cams, S, backend="numpy") == []
    with pytest.raises(ValueError, match="backend"):
        PC.render_point_clouds(meshes, cams, S, backend="cpu")


# ------------------------------------------------------------------------------------------------ prepare
def test_prepare_point_clouds_on_a_mesh_only_store(tmp_path):
    store = str(tmp_path / "meshes.zarr")
    meshes = [garment(s, n=3, drop=s) for s in range(3)]
    keys = write_mesh_only_store(store, meshes)
    args = ["--zarr_in", store, "--backend", "numpy", "--groups", "--batch_size", "2", "--point_clouds", "--pc_views", "4", "--pc_img_size", "32"]
    plain = P.main(["--zarr_in", store, "--backend", "numpy", "--groups"])
    samples = zarr_store.open_group(store, create=False)["samples"]
    assert plain["written"] == {} and not any("point_cloud" in samples[k] for k in keys)     # without the flag: no point_cloud group
    summary = P.main(args)
    assert summary["written"] == {"point_cloud": 3}
    cams = PC.camera_ring(AABB, 4, 32)
    first = {}
    for key, mesh in zip(keys, meshes):
        pc = samples[key]["point_cloud"]
        point, nocs, rgb, sizes = (pc[a][:] for a in PC.CLOUD_ARRAYS)
        first[key] = rgb
        assert (point.dtype, nocs.dtype, rgb.dtype, sizes.dtype) == (np.float32, np.float32, np.uint8, np.int64)
        assert point.shape == nocs.shape == rgb.shape == (len(point), 3) and sizes.shape == (4,) and sizes.sum() == len(point) and sizes.min() > 100
        want = PC.render_point_clouds([mesh], cams, 32, backend="numpy")[0]
        assert all(np.array_equal(pc[a][:], want[a]) for a in PC.CLOUD_ARRAYS)
        assert np.abs(to_sim(nocs).astype(np.float64) - point).max() <= LABEL_BOUND
        attrs = pc.attrs
        assert attrs["img_size"] == 32 and attrs["base_color"] == [0.5, 0.5, 0.5] and len(attrs["cameras"]) == 4
        assert np.array_equal(np.array(attrs["cameras"][1]["R"]), cams[1]["R"]) and attrs["cameras"][1]["near"] == cams[1]["near"]
    # a second run keeps the arrays, whatever colour it asks for; --overwrite rewrites them
    again = P.main(args + ["--pc_color", "1", "0", "0"])
    assert again["written"] == {"point_cloud": 0} and all(np.array_equal(samples[k]["point_cloud"]["rgb"][:], first[k]) for k in keys)
    over = P.main(args + ["--pc_color", "1", "0", "0", "--overwrite"])
    assert over["written"] == {"point_cloud": 3}
    for k in keys:
        rgb = samples[k]["point_cloud"]["rgb"][:]
        assert rgb.shape == first[k].shape and (rgb[:, 1:] == 0).all() and (rgb[:, 0] > first[k][:, 0]).all()
        assert samples[k]["point_cloud"].attrs["base_color"] == [1.0, 0.0, 0.0]
    # the dataset reads the result
    ds = GarmentInputDataset(store, num_pc_sample=128, num_views=2, static_epoch_seed=True, enable_augumentation=False)
    sample = ds[1]
    assert sample["pos"].shape == sample["y"].shape == sample["x"].shape == (128, 3) and sample["x"].max() <= 1.0
    base = get_base_data(1, data_io(samples[keys[1]]), num_pc_sample=128, num_views=2, static_epoch_seed=True)
    assert np.array_equal(base["pos"], sample["pos"]) and np.abs(to_sim(base["y"]).astype(np.float64) - base["pos"]).max() <= LABEL_BOUND


def test_prepare_names_the_garment_no_camera_sees(tmp_path):
    store = str(tmp_path / "away.zarr")
    sim, nocs, faces = garment(0)
    keys = write_mesh_only_store(store, [(sim, nocs, faces), (sim + np.float32([0, 0, 50.0]), nocs, faces)])
    with pytest.raises(ValueError, match=f"sample {keys[1]}: no camera sees"):
        P.prepare_store(store, groups=[], backend="numpy", point_clouds=True, pc_img_size=32, log=lambda row: None)
    with pytest.raises(SystemExit):
        P.main(["--zarr_in", store, "--backend", "numpy", "--groups", "--point_clouds", "--pc_img_size", "32", "--pc_distance", "0.01"])
