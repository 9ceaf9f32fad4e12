"""CPU: the training monitors' host side -- garmentnets_amd.visualize's numpy backend against the reference's renderer (tests/golden/ref_render.npz,
written by tests/golden/make_golden_render.py), get_vis_idxs, the PNG writer, the viridis table, and the three flags of the two training parsers.

The tolerance is zero: index images and fp32 colour images are np.array_equal to the reference's, because both sides are the same IEEE operations
(fp64 camera and depth, fp32 colour-map arithmetic, table look-ups)."""
import struct
import zlib

import numpy as np
import pytest

from garmentnets_amd import visualize as V
from render_cases import equal, golden_pairs, load_golden


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_golden(golden_dir)


def test_numpy_backend_equals_every_golden_image(golden):
    pairs = golden_pairs(golden, "numpy")
    assert len(pairs) == 37
    wrong = [name for name, ours, ref in pairs if not equal(ours, ref)]
    assert not wrong, wrong
    assert not np.all(golden["wnf_none/img"][..., 3]) and np.all(golden["wnf_none/img"] == np.float32([1, 1, 1, 0]))      # nothing selected: all default
    assert np.all(golden["empty/idx"] == 0xFFFFFFFF)


def test_get_vis_idxs_equals_the_reference(golden):
    for j, (batch_idx, batch_size, this, per, limit) in enumerate(golden["vis/args"].tolist()):
        got = V.get_vis_idxs(batch_idx, batch_size=batch_size, this_batch_size=this, vis_per_items=per, max_vis_per_epoch=limit)
        for key, val in zip(("global", "selected", "vis"), got):
            assert val == golden[f"vis/{j}/{key}"].tolist(), (j, key)
    assert V.get_vis_idxs(2, this_batch_size=3, vis_per_items=1, max_vis_per_epoch=100) == ([6, 7, 8], [0, 1, 2], [6, 7, 8])       # batch_size from this one


def test_png_round_trip_and_chunk_crcs(tmp_path):
    rng = np.random.RandomState(3)
    img = rng.rand(5, 7, 4).astype(np.float32) * 1.4 - 0.2                              # values below 0 and above 1 are clipped
    img[0, 0], img[0, 1] = (0.0, 1.0, 0.999, 254.999 / 255), (1.0 / 255, 0.5, 2.0, -1.0)
    path = tmp_path / "sub" / "a.png"
    V.write_png(str(path), img)
    want = np.trunc(np.clip(img.astype(np.float64), 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)
    assert want[0, 0].tolist() == [0, 255, 254, 254] and want[0, 1].tolist() == [1, 127, 255, 0]
    got = V.read_png(str(path))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    data = path.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, kinds = 8, []
    while pos < len(data):                                                              # every chunk: length, type, body, CRC-32 of type + body
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        kinds.append(kind)
        pos += 12 + n
    assert kinds == [b"IHDR", b"IDAT", b"IEND"] and pos == len(data)
    assert struct.unpack(">IIBBBBB", data[16:29]) == (7, 5, 8, 6, 0, 0, 0)              # 8-bit RGBA, no interlace
    raw = zlib.decompress(data[data.index(b"IDAT") + 4:-16])
    assert len(raw) == 5 * (1 + 7 * 4) and set(raw[::29]) == {0}                        # filter 0 on every row
    broken = bytearray(data)
    broken[40] ^= 1
    (tmp_path / "b.png").write_bytes(bytes(broken))
    with pytest.raises(ValueError, match="CRC"):
        V.read_png(str(tmp_path / "b.png"))
    V.write_png(str(tmp_path / "c.png"), want)                                          # uint8 goes through as it is
    assert np.array_equal(V.read_png(str(tmp_path / "c.png")), want)


def test_out_of_range_rules_that_are_ours():
    S = 16
    far = np.array([[-5.0, 0.5, 0.5], [0.5, 0.5, 7.0]], dtype=np.float32)               # c * (S - 1) <= -1: the reference's cast wraps, ours clamps to 0
    idx = V.render_points_idx(far, img_size=S, kernel_size=1, backend="numpy")
    assert idx[7, 0] == 0 and idx[0, 7] == 1 and np.count_nonzero(idx != 0xFFFFFFFF) == 2         # (front: y pixel from 1 - z, x pixel from x)
    huge = np.array([[3e9, 0.0, 1.0]], dtype=np.float32)                                # beyond 2^32: clamps to S - 1
    assert V.render_points_idx(huge, img_size=S, kernel_size=1, backend="numpy")[0, S - 1] == 0
    for side in V.SIDES:
        for axis in range(3):
            for bad in (np.nan, np.inf, -np.inf):                                       # (y = -inf on 'front' included: not drawn here)
                p = np.full((3, 3), 0.5, dtype=np.float32)
                p[1, axis] = bad
                idx = V.render_points_idx(p, img_size=S, kernel_size=4, side=side, backend="numpy")
                assert not np.any(idx == 1) and np.any(idx == 0) and not np.any(idx == 2), (side, axis, bad)      # 0 wins the tie with 2
    img = V.render_nocs(np.zeros((0, 3), np.float32), img_size=S, backend="numpy", default_color=(0.25, 0.5, 0.75, 1.0))
    assert img.shape == (S, S, 4) and np.all(img == np.float32([0.25, 0.5, 0.75, 1.0]))
    with pytest.raises(ValueError, match="side"):
        V.render_nocs(far, side="back", backend="numpy")
    with pytest.raises(ValueError, match="kernel_size"):
        V.render_nocs(far, img_size=S, kernel_size=S + 1, backend="numpy")


def test_viridis_against_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps["viridis"]
    lut = V.viridis_lut()
    assert lut.dtype == np.float32 and lut.shape == (256, 4)
    assert np.array_equal(lut[:, :3], np.asarray(cmap.colors, dtype=np.float64).astype(np.float32)) and np.all(lut[:, 3] == 1)
    x = np.concatenate([np.float32([-0.1, 0, 0.999, 1, 1.2, np.nan, np.inf, -np.inf, -0.0]), np.linspace(-0.2, 1.2, 1001, dtype=np.float32),
                        np.arange(257, dtype=np.float32) / np.float32(256)])
    for lo, hi in ((-0.5, 1.5), (0.0, 1.0)):
        xs = (x * np.float32(hi - lo) + np.float32(lo)).astype(np.float32)
        with np.errstate(invalid="ignore"):
            want = cmap((xs - lo) / (hi - lo)).astype(np.float32)                       # the reference's get_wnf_cmap, then its fp32 image
        assert np.array_equal(V.viridis(xs, lo, hi), want)


def test_both_parsers_accept_the_three_flags():
    from garmentnets_amd import train, train_pipeline
    flags = ["--vis_per_items", "2", "--max_vis_per_epoch_train", "5", "--max_vis_per_epoch_val", "3"]
    for mod, extra in ((train, ["--model", "pointnet2"]), (train_pipeline, [])):
        a = mod.parse_args(["--zarr_in", "x.zarr"] + extra + flags)
        assert (a.vis_per_items, a.max_vis_per_epoch_train, a.max_vis_per_epoch_val) == (2, 5, 3)
        a = mod.parse_args(["--zarr_in", "x.zarr"] + extra)
        assert (a.vis_per_items, a.max_vis_per_epoch_train, a.max_vis_per_epoch_val) == (None, None, None)       # None: the model's hyper-parameter
