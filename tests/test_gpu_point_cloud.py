"""GPU (-m gpu): the point clouds from meshes of csrc/render.hip (ops.depth_render_batch, ops.depth_cloud; point_cloud.render_point_clouds) against the
numpy restatement of point_cloud.py, bit for bit on the index images and on every output array; the entries' refusals; `python -m
garmentnets_amd.prepare --point_clouds` end to end.  tests/test_point_cloud_host.py holds the restatement itself to the definitions."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import _lib, ops, point_cloud as PC, prepare as P  # noqa: E402
from garmentnets_amd.io import zarr_store  # noqa: E402
from garmentnets_amd.io.dataset import GarmentInputDataset  # noqa: E402
from garmentnets_amd.io.resident import ResidentDataset  # noqa: E402
from test_point_cloud_host import garment, to_sim, write_mesh_only_store  # noqa: E402
from test_winding_host import AABB  # noqa: E402

DEV = "cuda:0"
ARRAYS = ("point", "nocs", "rgb", "sizes")


def one_face():
    nocs = np.array([[0.2, 0.3, 0.2], [0.8, 0.4, 0.5], [0.4, 0.7, 0.9]], dtype=np.float32)
    return to_sim(nocs), nocs, np.array([[0, 1, 2]], dtype=np.int32)


def ring(S, away=1):
    """four cameras, number `away` turned half round about its own y axis: it looks away from the garments and its images are empty"""
    cams = PC.camera_ring(AABB, 4, S, azimuth0=10.0)
    flip = np.diag([-1.0, 1.0, -1.0])
    cams[away] = {**cams[away], "R": flip @ cams[away]["R"], "t": flip @ cams[away]["t"]}
    return cams


def with_guards(mesh, cam):
    """the mesh plus faces that are never drawn: a bad index, a NaN vertex, a vertex behind `cam`'s near plane, a zero-area face"""
    sim, nocs, faces = mesh
    z = PC.to_camera(sim, cam)[0, 2]
    behind = sim[0] + (cam["near"] / 2 - z) * np.asarray(cam["R"])[2]
    verts = np.concatenate([sim, [[np.nan, 0.0, 0.0]], [behind]]).astype(np.float32)
    n = len(sim)
    guards = np.array([[0, 1, n + 2], [0, -1, 2], [0, 1, n], [3, 3, 4]], dtype=np.int32)
    return verts, np.concatenate([nocs, np.zeros((2, 3), np.float32)]), np.concatenate([guards, faces, [[n + 1, 1, 2]]]).astype(np.int32)


def same_bits(got, want, tag):
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        for k in ARRAYS:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (tag, g, k, a[k].shape, b[k].shape)
            assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), \
                (tag, g, k, np.argwhere(a[k] != b[k])[:5])


@pytest.fixture(scope="module")
def batch():
    """S -> (meshes, cameras, the restatement's clouds), computed once"""
    out = {}
    for S in (32, 40):
        cams = ring(S)
        meshes = [one_face(), garment(1), garment(2, n=7, drop=5)]
        assert len(meshes[2][2]) > 256                                  # crosses the LDS face tile
        out[S] = (meshes, cams, PC.render_point_clouds(meshes, cams, S, backend="numpy"))
    return out


@pytest.mark.parametrize("S", [40, 32])
def test_a_ragged_batch_bit_for_bit(batch, S):
    meshes, cams, want = batch[S]
    sizes = np.stack([w["sizes"] for w in want])
    assert (sizes[:, 1] == 0).all() and (np.delete(sizes, 1, axis=1) > 0).all(), sizes      # empty images in the MIDDLE of the batch, points around them
    got = PC.render_point_clouds(meshes, cams, S)
    same_bits(got, want, f"S={S}")
    # the index images themselves
    verts = torch.from_numpy(np.concatenate([m[0] for m in meshes])).to(DEV)
    faces = torch.from_numpy(np.concatenate([m[2] for m in meshes])).to(DEV)
    vseg, fseg = np.cumsum([0] + [len(m[0]) for m in meshes]), np.cumsum([0] + [len(m[2]) for m in meshes])
    mesh_of = np.repeat(np.arange(3), 4)
    idx = ops.depth_render_batch(verts, faces, vseg, fseg, mesh_of, cams * 3, S).cpu().numpy().view(np.uint32)
    for i, g in enumerate(mesh_of):
        ref = PC.render_depth_idx_numpy(meshes[g][0], meshes[g][2], cams[i % 4], S)
        assert np.array_equal(idx[i], ref), (i, np.argwhere(idx[i] != ref)[:5])
    print(f"[point_cloud] S={S}: points per view {sizes.tolist()}")


@pytest.mark.parametrize("S", [40, 32])
def test_guard_faces_bit_for_bit(batch, S):
    meshes, cams, want = batch[S]
    guarded = [with_guards(m, cams[0]) for m in meshes]
    got = PC.render_point_clouds(guarded, cams, S)
    same_bits(got, PC.render_point_clouds(guarded, cams, S, backend="numpy"), f"guards S={S}")
    for g, w in zip(got, want):                                            # in view 0 no guard is drawn (the other cameras may see the face that
        n = int(w["sizes"][0])                                             # reaches behind camera 0): the view is the unguarded mesh's, bit for bit
        assert g["sizes"][0] == n and all(np.array_equal(g[k][:n], w[k][:n]) for k in ("point", "nocs", "rgb"))


def test_two_calls_agree_and_an_image_does_not_depend_on_its_launch(batch):
    meshes, cams, _ = batch[40]
    a, b = PC.render_point_clouds(meshes, cams, 40), PC.render_point_clouds(meshes, cams, 40)
    same_bits(a, b, "repeat")
    same_bits(PC.render_point_clouds([meshes[1]], cams, 40), [a[1]], "alone")
    same_bits(PC.render_point_clouds(meshes[::-1], cams, 40)[::-1], a, "reversed")
    same_bits(PC.render_point_clouds([meshes[1]], cams[1:2], 40), [{"point": np.zeros((0, 3), np.float32), "nocs": np.zeros((0, 3), np.float32),
                                                                    "rgb": np.zeros((0, 3), np.uint8), "sizes": np.zeros(1, np.int64)}], "empty")
    assert PC.render_point_clouds([], cams, 40) == []


# ------------------------------------------------------------------------------------------------ refusals
GOOD_CAM = {"R": np.eye(3), "t": np.zeros(3), "f": 4.0, "c": 4.0, "near": 0.1}


def _raw(entry, vseg=(0, 4), fseg=(0, 4), mesh=(0,), cam=None, ambient=0.35, table_segments=None, tab=True, out=True, S=8, I=None, M=None, N=4):
    """the C entry itself on sentinel-filled outputs -> nothing (a refusal must leave them alone)"""
    n = len(mesh)
    vseg, fseg, mesh_of = np.asarray(vseg, np.int64), np.asarray(fseg, np.int64), np.asarray(mesh, np.int32)
    cam = {**GOOD_CAM, **(cam or {})}
    table = (_lib.DepthImage * n)()
    for i, e in enumerate(table):
        m = min(max(int(mesh_of[i]), 0), len(vseg) - 2)
        e.vert_begin, e.vert_end, e.face_begin, e.face_end = table_segments or (int(vseg[m]), int(vseg[m + 1]), int(fseg[m]), int(fseg[m + 1]))
        e.R[:], e.t[:] = [float(v) for v in np.asarray(cam["R"], np.float64).reshape(9)], [float(v) for v in np.asarray(cam["t"], np.float64)]
        e.f, e.c, e.znear, e.ambient = cam["f"], cam["c"], cam["near"], ambient
        e.base_color[:] = [0.5, 0.5, 0.5]
    verts = torch.zeros((4, 3), dtype=torch.float32, device=DEV)
    faces = torch.zeros((4, 3), dtype=torch.int32, device=DEV)
    tab_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    host = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    tabs = (ctypes.cast(table, ctypes.c_void_p), p(tab_dev)) if tab else (None, None)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    I = n if I is None else I
    M = len(vseg) - 1 if M is None else M
    if entry == "gn_depth_render_batch":
        res = [torch.full((n, S, S), 7, dtype=torch.int32, device=DEV)]
        args = (p(verts), p(faces), host(vseg), host(fseg), M, host(mesh_of), *tabs, I, S, p(res[0]) if out else None, stream)
    else:
        idx = torch.full((n, S, S), -1, dtype=torch.int32, device=DEV)
        row_off = torch.zeros(n * S + 1, dtype=torch.int64, device=DEV)
        res = [torch.full((4, 3), 7.0, dtype=torch.float32, device=DEV), torch.full((4, 3), 7.0, dtype=torch.float32, device=DEV),
               torch.full((4, 3), 7, dtype=torch.uint8, device=DEV)]
        outs = [p(r) for r in res] if out else [None, None, None]
        args = (p(idx), p(verts), p(verts), p(faces), host(vseg), host(fseg), M, host(mesh_of), *tabs, p(row_off), I, S, N, *outs, stream)
    try:
        _lib.call(entry, *args)
    finally:
        torch.cuda.synchronize()
        assert all(bool((r == 7).all()) for r in res), "a refused call wrote its output"


@pytest.mark.parametrize("entry", ["gn_depth_render_batch", "gn_depth_cloud_write"])
def test_every_refusal_by_name_before_any_launch(entry):
    nan, inf = float("nan"), float("inf")
    bad_R = np.eye(3)
    bad_R[1, 2] = inf
    cases = [(dict(tab=False), "null pointer"),
             (dict(out=False), "null pointer" if entry == "gn_depth_render_batch" else "null output"),
             (dict(vseg=[4, 2]), "vseg is not a non-decreasing CSR"),
             (dict(vseg=[-1, 2]), "vseg is not a non-decreasing CSR"),
             (dict(fseg=[3, 1]), "fseg is not a non-decreasing CSR"),
             (dict(fseg=[0, 2 ** 32 - 1]), "fewer than 2\\^32 - 1"),
             (dict(table_segments=(0, 4, 0, 3)), "the table's segments differ from vseg / fseg"),
             (dict(vseg=[0, 2, 4], fseg=[0, 2, 4], mesh=(0, 1), table_segments=(0, 2, 0, 2)), "image 1: the table's segments differ"),
             (dict(mesh=(1,)), "mesh=1 outside \\[0, M=1\\)"),
             (dict(mesh=(-1,)), "mesh=-1 outside"),
             (dict(cam={"near": 0.0}), "near=0 is not positive and finite"),
             (dict(cam={"near": -1.0}), "near=-1 is not positive"),
             (dict(cam={"near": inf}), "near=inf is not positive and finite"),
             (dict(cam={"near": nan}), "near=nan is not positive"),
             (dict(cam={"R": bad_R}), "camera entry R\\[5\\]=inf is not finite"),
             (dict(cam={"t": [0.0, nan, 0.0]}), "camera entry t\\[1\\]=nan is not finite"),
             (dict(cam={"c": nan}), "camera entry c=nan is not finite"),
             (dict(cam={"f": 0.0}), "f=0 is not a positive finite focal length"),
             (dict(cam={"f": -2.0}), "f=-2 is not a positive"),
             (dict(cam={"f": inf}), "f=inf is not a positive finite"),
             (dict(ambient=1.5), "ambient=1.5 outside \\[0, 1\\]"),
             (dict(ambient=-0.25), "ambient=-0.25 outside \\[0, 1\\]"),
             (dict(ambient=nan), "ambient=nan outside"),
             (dict(S=0), "image size S=0 outside"),
             (dict(S=_lib.RENDER_MAX_SIZE + 1), "image size S=4097 outside"),
             (dict(I=65536), "I=65536 images outside")]
    if entry == "gn_depth_cloud_write":
        cases.append((dict(N=-1), "N=-1 rows"))
    for kw, words in cases:
        with pytest.raises(ValueError, match=entry + ": .*" + words):
            _raw(entry, **kw)
    _raw(entry, I=0)                                                       # no images: a no-op, nothing is written
    _raw(entry, I=0, tab=False)


def test_the_offsets_entry_refuses_and_counts():
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    S, n = 70, 3                                                           # a row longer than a wave
    rng = np.random.default_rng(0)
    img = np.where(rng.random((n, S, S)) < 0.3, rng.integers(0, 5, (n, S, S)), -1).astype(np.int32)
    img[1] = -1                                                            # an empty image in the middle
    idx = torch.from_numpy(img).to(DEV)
    row_off = torch.full((n * S + 1,), -7, dtype=torch.int64, device=DEV)
    sizes = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    for args, words in (((None, n, S, p(row_off), p(sizes)), "null pointer"), ((p(idx), n, S, None, p(sizes)), "null pointer"),
                        ((p(idx), n, 0, p(row_off), p(sizes)), "image size S=0 outside"), ((p(idx), 65536, S, p(row_off), p(sizes)), "I=65536 images")):
        with pytest.raises(ValueError, match="gn_depth_cloud_offsets: .*" + words):
            _lib.call("gn_depth_cloud_offsets", *args, stream)
    _lib.call("gn_depth_cloud_offsets", p(idx), 0, S, p(row_off), p(sizes), stream)
    torch.cuda.synchronize()
    assert bool((row_off == -7).all()) and bool((sizes == -7).all())
    _lib.call("gn_depth_cloud_offsets", p(idx), n, S, p(row_off), p(sizes), stream)
    counts = (img != -1).sum(axis=2).reshape(-1)
    assert np.array_equal(row_off.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))
    assert np.array_equal(sizes.cpu().numpy(), (img != -1).sum(axis=(1, 2))) and int(sizes[1]) == 0


def test_ops_refuse_what_would_size_an_access():
    verts = torch.zeros((4, 3), dtype=torch.float32, device=DEV)
    faces = torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="ends beyond its tensor"):
        ops.depth_render_batch(verts, faces, [0, 5], [0, 2], [0], [GOOD_CAM], 8)
    with pytest.raises(ValueError, match="mesh number is outside"):
        ops.depth_render_batch(verts, faces, [0, 4], [0, 2], [1], [GOOD_CAM], 8)
    with pytest.raises(ValueError, match="near=0 is not positive"):
        ops.depth_render_batch(verts, faces, [0, 4], [0, 2], [0], [{**GOOD_CAM, "near": 0.0}], 8)
    with pytest.raises(ValueError, match="image size S=0"):
        ops.depth_render_batch(verts, faces, [0, 4], [0, 2], [0], [GOOD_CAM], 0)
    with pytest.raises(TypeError):
        ops.depth_render_batch(verts, faces.long(), [0, 4], [0, 2], [0], [GOOD_CAM], 8)
    idx = ops.depth_render_batch(verts, faces, [0, 4], [0, 2], [0], [GOOD_CAM], 8)
    assert bool((idx == -1).all())                                         # every vertex at the camera: behind its near plane
    with pytest.raises(ValueError, match="expected \\(4, 3\\) nocs"):
        ops.depth_cloud(idx, verts, verts[:3].contiguous(), faces, [0, 4], [0, 2], [0], [GOOD_CAM])
    with pytest.raises(ValueError, match="ambient=2 outside"):
        ops.depth_cloud(idx, verts, verts, faces, [0, 4], [0, 2], [0], [GOOD_CAM], ambients=[2.0])
    point, label, rgb, sizes = ops.depth_cloud(idx, verts, verts, faces, [0, 4], [0, 2], [0], [GOOD_CAM])
    assert point.shape == label.shape == rgb.shape == (0, 3) and sizes.tolist() == [0]
    assert ops.depth_render_batch(verts, faces, [0, 4], [0, 2], [], [], 8).shape == (0, 8, 8)


# ------------------------------------------------------------------------------------------------ prepare, end to end
def test_prepare_point_clouds_equals_the_numpy_backend_and_feeds_the_resident_dataset(tmp_path):
    meshes = [garment(3, n=3, drop=2), garment(4, n=7, drop=1)]
    stores = {}
    for backend in ("hip", "numpy"):
        stores[backend] = str(tmp_path / f"{backend}.zarr")
        keys = write_mesh_only_store(stores[backend], meshes)
        summary = P.main(["--zarr_in", stores[backend], "--backend", backend, "--groups", "--point_clouds", "--pc_img_size", "40"])
        assert summary["written"] == {"point_cloud": 2}
    a, b = (zarr_store.open_group(stores[k], create=False)["samples"] for k in ("hip", "numpy"))
    for key in keys:
        for name in ARRAYS:
            x, y = a[key]["point_cloud"][name][:], b[key]["point_cloud"][name][:]
            assert x.dtype == y.dtype and np.array_equal(x, y), (key, name)
        assert a[key]["point_cloud"].attrs == b[key]["point_cloud"].attrs and a[key]["point_cloud"]["sizes"][:].min() > 100
    ds = GarmentInputDataset(stores["hip"], num_pc_sample=128, num_views=2, static_epoch_seed=True, enable_augumentation=False)
    chunk = [1, 0]
    host = GarmentInputDataset.collate([ds[k] for k in chunk])
    got = ResidentDataset(ds, [0, 1], DEV).batch(chunk)
    assert set(got.keys) == set(host.keys) and got.sizes == host.sizes
    for k in host.keys:
        assert torch.equal(getattr(got, k).cpu(), getattr(host, k)), k
    assert got.pos.shape == (256, 3) and np.abs(to_sim(got.y.cpu().numpy()).astype(np.float64) - got.pos.cpu().numpy()).max() <= 2e-7
