"""GPU (-m gpu): the mesh rasteriser of csrc/render.hip (ops.render_mesh_batch, ops.color_mesh_batch) against the numpy restatement of
visualize.py, bit for bit on the index image and on the RGBA image; the entries' refusals; `python -m garmentnets_amd.evaluate` with the
visualisation flags end to end.  tests/test_mesh_render_host.py holds the restatement itself to an exact oracle."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import _lib, evaluate as E, ops, visualize as V  # noqa: E402
from garmentnets_amd.io import zarr_store  # noqa: E402

DEV = "cuda:0"
NONE = 0xFFFFFFFF
SIZES = (17, 33, 40)                                # S - 1 a power of two twice (vertices land on samples exactly); 40 is no multiple of the tile


def point(cx, cy, depth, side="front"):
    """the point that the camera of `side` puts at the camera coordinates (cx, cy, depth)"""
    return {"front": [cx, depth, 1 - cy], "top": [cx, 1 - cy, 1 - depth], "left": [depth, 1 - cx, 1 - cy]}[side]


def spec(cam_verts, faces, side="front", seed=0, **kw):
    verts = np.array([point(*v, side=side) for v in cam_verts], dtype=np.float32).reshape(-1, 3)
    colors = np.random.default_rng(seed).random((len(verts), 4)).astype(np.float32)
    return V.mesh_spec(verts, np.asarray(faces, dtype=np.int32).reshape(-1, 3), colors, side=side, **kw)


def both(specs, S):
    """(index images, RGBA images) of the device, after asserting that the numpy backend gives the same bits"""
    idx = V.render_mesh_idx_batch(specs, S, "device")
    ref = V.render_mesh_idx_batch(specs, S, "numpy")
    assert idx.dtype == ref.dtype == np.uint32 and np.array_equal(idx, ref), np.argwhere(idx != ref)[:5]
    img = V.render_mesh_batch(specs, S, "device")
    want = V.render_mesh_batch(specs, S, "numpy")
    assert img.dtype == want.dtype == np.float32 and np.array_equal(img.view(np.uint32), want.view(np.uint32)), np.argwhere(img != want)[:5]
    return idx, img


TRI = [(0.125, 0.125, 0.5), (0.875, 0.25, 0.25), (0.25, 0.875, 0.75)]
QUAD = [(0.25, 0.25, 0.5), (0.75, 0.25, 0.5), (0.75, 0.75, 0.25), (0.25, 0.75, 0.5)]       # its corners and its diagonal lie on pixel samples


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("side", ["front", "top", "left"])
def test_hand_cases_bit_for_bit(S, side):
    g = (S - 1 + 0.5) / (S - 1)                      # the camera coordinate of the last sample
    quad = [((round(x * (S - 1)) + 0.5) / (S - 1), (round(y * (S - 1)) + 0.5) / (S - 1), z) for x, y, z in QUAD]
    far = 2.0 ** 24 / (256 * (S - 1)) * 1.5          # its fixed-point coordinate passes 2^24
    cases = {
        "one face": spec(TRI, [[0, 1, 2]], side),
        "a negatively oriented face": spec(TRI, [[0, 2, 1]], side),
        "two faces sharing an edge on samples": spec(quad, [[0, 1, 2], [0, 2, 3]], side),
        "the same, one of them turned": spec(quad, [[0, 1, 2], [0, 3, 2]], side),
        "two identical coplanar faces": spec(TRI + TRI, [[3, 4, 5], [0, 1, 2]], side),
        "a zero-area face first": spec(TRI + [(0.5, 0.5, 0.0)], [[0, 3, 3], [0, 0, 1], [0, 1, 2]], side),
        "a NaN vertex": spec(TRI + [(np.nan, 0.5, 0.0)], [[0, 1, 2], [0, 1, 3]], side),
        "indices V and -1": spec(TRI, [[0, 1, 2], [0, 1, 3], [0, -1, 2], [-2 ** 31, 1, 2], [2 ** 31 - 1, 1, 2]], side),
        "partly and wholly outside": spec([(-0.5, 0.25, 0.5), (0.5, -0.25, 0.5), (0.5, 0.75, 0.5), (1.5, 1.5, 0.5), (2.5, 1.5, 0.5), (1.5, 2.5, 0.5),
                                           (g - 0.01, g - 0.01, 0.5), (1.5, g - 0.01, 0.5), (g - 0.01, 1.5, 0.5)], [[0, 1, 2], [3, 4, 5], [6, 7, 8]], side),
        "beyond 2^24": spec(TRI + [(far, 0.5, 0.0), (-far, 0.5, 0.0)], [[0, 1, 2], [0, 1, 3], [4, 1, 2]], side),
        "no faces": spec(TRI, np.zeros((0, 3), np.int32), side),
        "no vertices": spec([], [[0, 1, 2]], side),
    }
    idx, img = both(list(cases.values()), S)
    got = dict(zip(cases, idx))
    one = got["one face"]
    assert np.count_nonzero(one == 0) > S * S // 8 and set(np.unique(one)) == {0, NONE}
    assert np.array_equal(got["a negatively oriented face"], one)                           # two-sided
    shared = got["two faces sharing an edge on samples"]
    assert np.array_equal(shared != NONE, got["the same, one of them turned"] != NONE)
    if S in (17, 33):                                # half-open in x and in y: the quad's samples less one owned column and one owned row
        n = round(0.5 * (S - 1))
        assert np.count_nonzero(shared != NONE) == n * n
    assert set(np.unique(got["two identical coplanar faces"])) == {0, NONE}                 # equal depths: the lowest index
    assert np.array_equal(got["a zero-area face first"] == 2, one == 0) and set(np.unique(got["a zero-area face first"])) == {2, NONE}
    for name in ("a NaN vertex", "indices V and -1", "beyond 2^24"):                        # not drawn, and the rest of the image is unchanged
        assert np.array_equal(got[name], one), name
    outside = got["partly and wholly outside"]
    assert set(np.unique(outside)) == {0, 2, NONE} and outside[S - 1, S - 1] == 2 and np.count_nonzero(outside == 2) == 1
    assert (got["no faces"] == NONE).all() and (got["no vertices"] == NONE).all()
    assert np.array_equal(img[list(cases).index("no faces")], np.broadcast_to(np.float32([1, 1, 1, 0]), (S, S, 4)))


def soup(S, seed=3, n=600):
    """600 faces, three LDS tiles: small triangles all over and beyond the view (every pixel tile keeps some and drops others, interleaved), the
    last face large and nearest to the camera"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.3, 1.3, (n, 1, 2))
    xy = centre + rng.uniform(-0.12, 0.12, (n, 3, 2))
    z = rng.uniform(0.2, 0.9, (n, 3, 1))
    cam = np.concatenate([xy, z], axis=2).reshape(-1, 3)
    cam[-3:] = [(0.3, 0.3, 0.05), (0.8, 0.4, 0.05), (0.4, 0.8, 0.05)]
    faces = np.arange(3 * n).reshape(n, 3)
    faces[::7] = faces[::7, ::-1]                    # some stored the other way round
    return [tuple(v) for v in cam], faces


@pytest.mark.parametrize("S", SIZES)
def test_600_faces_cross_three_lds_tiles(S):
    cam, faces = soup(S)
    idx, _ = both([spec(cam, faces, "front", ambient=0.2, default_color=(0.1, 0.2, 0.3, 1.0))], S)
    drawn = idx[0][idx[0] != NONE]
    assert (drawn == 599).sum() > S * S // 16 and (drawn < 256).any() and ((drawn >= 256) & (drawn < 512)).any()
    assert len(np.unique(drawn)) > 40


def test_huge_coplanar_faces_are_decided_by_the_last_bit_of_the_depth():
    """Twelve faces far larger than the view, all in the plane depth = (x + 2 y) / 3 exactly (vertices on a 2^-13 lattice with x + 2 y = 0 mod 3, so
    S = 33 puts them on fixed-point coordinates up to 2^24 without rounding).  At a sample the exact depth is one real number, not a dyadic one, and
    every face computes its own rounding of it from weights of 45 bits whose products with the depths round: the winner is whoever rounds lowest.
    Emulated on the host with exact fractions, a depth with any one multiply-add fused changes the winner at 370 to 750 of the 1089 pixels."""
    S, n = 33, 12
    rng = np.random.default_rng(0)
    cam = []
    for _ in range(n):
        phase = rng.uniform(0, 2 * np.pi)
        for j in range(3):
            ang, rad = phase + 2 * np.pi * j / 3 + rng.uniform(-0.4, 0.4), rng.uniform(300, 1500)
            kx, ky = int(rad * np.cos(ang) * 8192), int(rad * np.sin(ang) * 8192)
            kx -= (kx + 2 * ky) % 3
            cam.append((kx / 8192, ky / 8192, (kx + 2 * ky) // 3 / 8192))
    s = spec(cam, np.arange(3 * n).reshape(n, 3))
    assert np.array_equal(V.to_camera(s["verts"], "front"), np.array(cam))                  # exact in fp32
    idx, _ = both([s], S)
    winners, counts = np.unique(idx[0], return_counts=True)
    assert len(winners) == n and NONE not in winners and counts.min() >= 5 and counts.max() < S * S // 2


def test_a_ragged_batch_equals_its_single_launches_and_repeats():
    S = 40
    cam, faces = soup(S, seed=4)
    specs = [spec(cam, faces, "top", seed=1), spec(TRI, [[0, 2, 1]], "left", seed=2, ambient=0.0), spec(cam[:300], faces[:100], "front", seed=3),
             spec(TRI, np.zeros((0, 3), np.int32), "front")]
    idx, img = both(specs, S)
    for i, s in enumerate(specs):
        assert np.array_equal(V.render_mesh_idx_batch([s], S)[0], idx[i]), i
        assert np.array_equal(V.render_mesh_batch([s], S)[0].view(np.uint32), img[i].view(np.uint32)), i
    again = V.render_mesh_batch(specs[::-1], S)[::-1]
    assert np.array_equal(again.view(np.uint32), img.view(np.uint32))
    assert np.array_equal(V.render_mesh_batch(specs, S).view(np.uint32), img.view(np.uint32))
    assert V.render_mesh_batch([], S).shape == (0, S, S, 4) and V.render_mesh_idx_batch([], S).shape == (0, S, S)


# ------------------------------------------------------------------------------------------------ refusals
def _raw(entry, vseg, fseg, sides=(0,), ambients=(0.35,), tab=True, out=True, S=8, I=None):
    """the C entry itself on a sentinel-filled output -> the output afterwards (a refusal must leave it alone)"""
    n = len(sides)
    vseg, fseg = np.asarray(vseg, np.int64), np.asarray(fseg, np.int64)
    table = (_lib.MeshImage * n)()
    for i, e in enumerate(table):
        e.vert_begin, e.vert_end, e.face_begin, e.face_end = int(vseg[i]), int(vseg[i + 1]), int(fseg[i]), int(fseg[i + 1])
        e.side, e.ambient = sides[i], ambients[i]
    verts = torch.zeros((4, 3), dtype=torch.float32, device=DEV)
    faces = torch.zeros((4, 3), dtype=torch.int32, device=DEV)
    colors = torch.zeros((4, 4), dtype=torch.float32, device=DEV)
    tab_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    host = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    tabs = (ctypes.cast(table, ctypes.c_void_p), p(tab_dev)) if tab else (None, None)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    I = n if I is None else I
    if entry == "gn_render_mesh_batch":
        res = torch.full((n, S, S), 7, dtype=torch.int32, device=DEV)
        args = (p(verts), p(faces), host(vseg), host(fseg), *tabs, I, S, p(res) if out else None, stream)
    else:
        idx = torch.full((n, S, S), -1, dtype=torch.int32, device=DEV)
        res = torch.full((n, S, S, 4), 7.0, dtype=torch.float32, device=DEV)
        args = (p(idx), p(verts), p(faces), p(colors), host(vseg), host(fseg), *tabs, I, S, p(res) if out else None, stream)
    try:
        _lib.call(entry, *args)
    finally:
        torch.cuda.synchronize()
        assert (res == 7).all(), "a refused call wrote its output"
    return res


@pytest.mark.parametrize("entry", ["gn_render_mesh_batch", "gn_color_mesh_batch"])
def test_every_refusal_by_name_before_any_launch(entry):
    for kw, words in ((dict(vseg=[0, 4], fseg=[0, 4], tab=False), "null pointer"),
                      (dict(vseg=[0, 4], fseg=[0, 4], out=False), "null pointer"),
                      (dict(vseg=[4, 2], fseg=[0, 4]), "vseg is not a non-decreasing CSR"),
                      (dict(vseg=[-1, 2], fseg=[0, 4]), "vseg is not a non-decreasing CSR"),
                      (dict(vseg=[0, 4], fseg=[3, 1]), "fseg is not a non-decreasing CSR"),
                      (dict(vseg=[0, 4], fseg=[0, 2 ** 32 - 1]), "fewer than 2\\^32 - 1"),
                      (dict(vseg=[0, 4], fseg=[0, 4], sides=(3,)), "side=3 outside"),
                      (dict(vseg=[0, 4], fseg=[0, 4], sides=(-1,)), "side=-1 outside"),
                      (dict(vseg=[0, 4], fseg=[0, 4], ambients=(1.5,)), "ambient=1.5 outside \\[0, 1\\]"),
                      (dict(vseg=[0, 4], fseg=[0, 4], ambients=(-0.25,)), "ambient=-0.25 outside \\[0, 1\\]"),
                      (dict(vseg=[0, 4], fseg=[0, 4], ambients=(float("nan"),)), "ambient=nan outside"),
                      (dict(vseg=[0, 4], fseg=[0, 4], S=0), "image size S=0 outside"),
                      (dict(vseg=[0, 4], fseg=[0, 4], S=_lib.RENDER_MAX_SIZE + 1), "image size S=4097 outside"),
                      (dict(vseg=[0, 4], fseg=[0, 4], I=65536), "I=65536 images outside")):
        with pytest.raises(ValueError, match=entry + ": .*" + words):
            _raw(entry, **kw)
    _raw(entry, vseg=[0, 4], fseg=[0, 4], I=0)                                               # no images: a no-op, nothing is written
    _raw(entry, vseg=[0, 4], fseg=[0, 4], I=0, tab=False)


def test_ops_refuse_what_would_size_an_access():
    verts = torch.zeros((4, 3), dtype=torch.float32, device=DEV)
    faces = torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="ends beyond its tensor"):
        ops.render_mesh_batch(verts, faces, [0, 5], [0, 2], ["front"], 8)
    with pytest.raises(ValueError, match="ends beyond its tensor"):
        ops.render_mesh_batch(verts, faces, [0, 4], [0, 3], ["front"], 8)
    with pytest.raises(ValueError, match="side=7 outside"):
        ops.render_mesh_batch(verts, faces, [0, 4], [0, 2], [7], 8)
    with pytest.raises(ValueError, match="image size S=0"):
        ops.render_mesh_batch(verts, faces, [0, 4], [0, 2], ["front"], 0)
    with pytest.raises(TypeError):
        ops.render_mesh_batch(verts, faces.long(), [0, 4], [0, 2], ["front"], 8)
    idx = ops.render_mesh_batch(verts, faces, [0, 4], [0, 2], ["front"], 8)
    with pytest.raises(ValueError, match="ambient=2 outside"):
        ops.color_mesh_batch(idx, verts, faces, torch.zeros((4, 4), device=DEV), [0, 4], [0, 2], ["front"], ambients=[2.0])
    with pytest.raises(ValueError, match="expected \\(4, 4\\) colors"):
        ops.color_mesh_batch(idx, verts, faces, torch.zeros((3, 4), device=DEV), [0, 4], [0, 2], ["front"])
    assert ops.render_mesh_batch(verts, faces, [0], [0], [], 8).shape == (0, 8, 8)


# ------------------------------------------------------------------------------------------------ evaluate end to end
def test_evaluate_writes_the_ranked_panels(tmp_path):
    from garmentnets_amd import predict as PR
    from test_gpu_evaluate import write_dataset
    din, dout = str(tmp_path / "dataset.zarr"), str(tmp_path / "prediction.zarr")
    write_dataset(din, 3)
    PR.main(["--zarr_in", din, "--zarr_out", dout, "--num_pc_sample", "1800", "--num_views", "3", "--grid", "16", "--volume_size", "24",
             "--auto_level", "--static_epoch_seed", "--subset", "all"])
    root = zarr_store.open_group(dout, create=False)
    keys = root["samples"].keys()
    root["samples"][keys[1]]["marching_cubes_mesh"].array("volume_gradient_magnitude", np.full(1, np.nan, dtype=np.float32))     # a null sample
    S = 40
    args = ["--prediction", dout, "--zarr_in", din, "--num_points", "2000"]
    flags = ["--vis_samples_per_instance", "1", "--vis_num_normal", "1", "--vis_num_best", "1", "--vis_num_worst", "1", "--vis_img_size", str(S),
             "--vis_sides", "front", "top"]
    plain = E.main(args + ["--output_dir", str(tmp_path / "plain")])
    out = E.main(args + flags + ["--output_dir", str(tmp_path / "vis")])
    assert plain["errors"] == [] and out["errors"] == [] and "vis_files" not in plain
    assert not os.path.exists(tmp_path / "plain" / "vis")
    for f in ("all_metrics.csv", "all_metrics_agg.csv", "summary.json"):
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "vis" / f, "rb").read(), f
    # the expected names: the null sample ranks last (NaN), so it is the worst; row 0 is regular unless it is the best
    labels = E.vis_selection(out["table"][E.DEFAULT_RANK_METRIC], 1, 1, 1, 1)
    assert labels[1] == "worst_00" and "best_00" in labels.values()
    want = sorted(f"{func}_{label}.png" for func in E.VIS_FUNCS for label in labels.values())
    assert sorted(os.listdir(tmp_path / "vis" / "vis")) == want
    # the numpy backend's images of the same panels
    sim_aabb = np.asarray(zarr_store.open_group(din, create=False)["summary"]["cloth_aabb_union"])
    samples = [root["samples"][k] for k in keys]
    E.write_vis(str(tmp_path / "numpy"), samples, out["is_null"], labels, sim_aabb, sides=("front", "top"), img_size=S, vis_backend="numpy",
                value_threshold=E.resolve_threshold(root, E.DEFAULT_THRESHOLD_PATH))
    panels = {"task_mesh_vis": 3, "nocs_mesh_vis": 2, "nocs_pc_vis": 3}
    covered = 0
    for name in want:
        img = V.read_png(str(tmp_path / "vis" / "vis" / name))
        assert img.shape == (2 * S, panels[name.split("_vis_")[0] + "_vis"] * S, 4), name
        assert np.array_equal(img, V.read_png(str(tmp_path / "numpy" / "vis" / name))), name
        covered += int((img[:, :, 3] > 0).sum())
        if "mesh_vis_worst" in name:                 # the null sample: its predicted mesh panel is background
            assert (img[:, S:2 * S, 3] == 0).all() and (img[S:, :S, 3] > 0).any(), name
    assert covered > 20 * S
