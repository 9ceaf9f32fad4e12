"""GPU (-m gpu): the training monitors on the device -- csrc/render.hip through ops.render_points_batch / ops.color_idx_batch and
garmentnets_amd.visualize's device backend -- against the numpy backend and the reference's renderer (tests/golden/ref_render.npz), and both training
loops with --vis_per_items.

The tolerance is zero everywhere: the kernels and the numpy restatement are the same IEEE operations (fp64 camera, pixel and depth; fp32 colour-map
arithmetic; table look-ups), and the winner of a pixel has an order-free definition.

Shapes: S = 8 (half a pixel tile), 20 (a ragged second tile), 256; per-image N = 0, 1, 255, 256, 257 around the 256-point staging tile; k = 1, 4, 5, 8
and k = S; every side.  All images of one size go through ONE launch pair, so the ragged batch itself is under test."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import _lib, ops, visualize as V  # noqa: E402
from render_cases import equal, golden_pairs, load_golden  # noqa: E402

DEV = "cuda:0"
SIDES = ("front", "top", "left")
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_golden(golden_dir)


# ------------------------------------------------------------------------------------------------ 1. the golden inputs
def test_device_equals_numpy_and_the_reference_on_the_golden_inputs(golden):
    dev, host = golden_pairs(golden, "device"), golden_pairs(golden, "numpy")
    assert len(dev) == 37
    wrong = [name for (name, ours, ref), (_, restated, _) in zip(dev, host) if not (equal(ours, ref) and equal(ours, restated))]
    assert not wrong, wrong
    # the slice taken by torch on the device selects what numpy selects, its open ends included
    q, wnf = torch.from_numpy(golden["wnf_none/query"]).to(DEV), torch.from_numpy(golden["wnf/values"]).to(DEV)
    assert equal(V.render_wnf_points(q, wnf, img_size=32), golden["wnf_none/img"])
    q = torch.from_numpy(golden["wnf/query"]).to(DEV)
    assert equal(V.render_wnf_points_pair(q, wnf, torch.from_numpy(golden["wnf_pair/pred"]).to(DEV), img_size=32), golden["wnf_pair/img"])


# ------------------------------------------------------------------------------------------------ 2. the kernel's edges
def _cloud(rng, n, kind="cube"):
    p = rng.rand(n, 3).astype(np.float32)
    if kind == "pixel":                                  # every point in one pixel (of every side), distinct and equal depths among them
        p = (np.float32(0.4) + p * np.float32(1e-3)).astype(np.float32)
        p[n // 2:] = p[:n - n // 2]
    elif kind == "border":                               # every point on an edge of the image, whatever the side
        p[np.arange(n), rng.randint(0, 3, n)] = rng.randint(0, 2, n).astype(np.float32)
        p[np.arange(n), rng.randint(0, 3, n)] = rng.randint(0, 2, n).astype(np.float32)
    else:
        p[: n // 8] = p[n // 8: 2 * (n // 8)]            # repeated points: equal depths, the lowest index wins
        p[-(n // 16 + 1):, 0] = np.float32(-0.3)         # left of every image of 'front' / 'top', and a few past the far side
        p[: n // 16, 2] = np.float32(1.7)
    return p


def _edge_cases(S, seed):
    rng = np.random.RandomState(seed)
    ks = [k for k in (1, 4, 5, 8) if k <= S]
    sides = itertools.cycle(SIDES)
    cases = [(_cloud(rng, n), next(sides), k) for n in (0, 1, 255, 256, 257) for k in ks]
    cases += [(_cloud(rng, 257), side, 4) for side in SIDES]
    cases += [(_cloud(rng, n), side, S) for n, side in ((1, "front"), (3, "left"))]
    cases += [(_cloud(rng, 300, "pixel"), side, 4) for side in SIDES] + [(_cloud(rng, 300, "border"), side, k) for side, k in zip(SIDES, (1, 4, 5))]
    return cases


@pytest.mark.parametrize("S", [8, 20, 256])
def test_device_equals_numpy_at_the_kernel_edges(S):
    cases = _edge_cases(S, 100 + S)
    points, sides, ks = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    want = V.render_idx_batch(points, sides, ks, S, backend="numpy")
    got = V.render_idx_batch(points, sides, ks, S, backend="device")
    assert got.dtype == np.uint32 and got.shape == (len(cases), S, S)
    wrong = [(i, len(points[i]), sides[i], ks[i]) for i in range(len(cases)) if not np.array_equal(got[i], want[i])]
    assert not wrong, wrong
    assert np.all(got[0] == NONE) and np.any(got[-1] != NONE)
    # colours: a table, the points themselves, scalars through viridis with values outside the range and NaN, another default, overlays
    rng = np.random.RandomState(S)
    specs = []
    for j, (p, side, k) in enumerate(cases):
        n = len(p)
        over = [(rng.rand(3).astype(np.float32), (1, 0, 0, 1), min(2 * k, S)), (rng.rand(3).astype(np.float32), (0, 1, 0, 0.5), k),
                (np.float32([np.nan, 0.5, 0.5]), (0, 0, 1, 1), k)][: j % 4]
        if j % 3 == 0:
            vals = (rng.rand(n) * 3 - 1).astype(np.float32)
            vals[::7] = np.nan
            specs.append(V.image_spec(p, side, k, values=vals, vrange=V.WNF_RANGE, overlays=over))
        elif j % 3 == 1:
            specs.append(V.image_spec(p, side, k, colors=rng.rand(n, 4).astype(np.float32), default_color=(0.1, 0.2, 0.3, 0.4), overlays=over))
        else:
            specs.append(V.image_spec(p, side, k, overlays=over))
    want, got = V.render_batch(specs, S, backend="numpy"), V.render_batch(specs, S, backend="device")
    wrong = [j for j in range(len(specs)) if not equal(got[j], want[j])]
    assert not wrong, wrong


def test_a_ragged_batch_equals_its_single_launches_and_repeats_bit_for_bit():
    S = 20
    cases = _edge_cases(S, 7)
    pts = [torch.from_numpy(c[0]).to(DEV) for c in cases]
    seg = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])])
    joint = torch.cat(pts).contiguous()
    sides, ks = [c[1] for c in cases], [c[2] for c in cases]
    a = ops.render_points_batch(joint, seg, sides, ks, S)
    b = ops.render_points_batch(joint, seg, sides, ks, S)
    assert a.dtype == torch.int32 and torch.equal(a, b)
    for i, p in enumerate(pts):
        one = ops.render_points_batch(p.contiguous(), [0, len(p)], [sides[i]], [ks[i]], S)
        assert torch.equal(one[0], a[i]), i
    values = torch.rand(int(seg[-1]), device=DEV)
    images = [{"offset": int(seg[i]), "count": int(seg[i + 1] - seg[i]), "mode": "viridis", "side": sides[i], "vmin": 0.0, "vmax": 1.0,
               "overlays": [((0.5, 0.5, 0.5), (1, 0, 0, 1), ks[i])]} for i in range(len(cases))]
    c = ops.color_idx_batch(a, images, values=values)
    assert torch.equal(c, ops.color_idx_batch(a, images, values=values))
    for i in (0, 5, len(cases) - 1):
        one = ops.color_idx_batch(a[i:i + 1].contiguous(), [dict(images[i])], values=values)
        assert torch.equal(one[0], c[i]), i


# ------------------------------------------------------------------------------------------------ 3. refusals, by name
def _host(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _entry(seg, side, k, S, I=None):
    """gn_render_points_batch called directly with HOST tables that the entry refuses before it launches anything"""
    keep = [_host(seg, np.int64), _host(side, np.int32), _host(k, np.int32)]
    tab, out, pts = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(3, device=DEV)
    return _lib.call("gn_render_points_batch", pts.data_ptr(), keep[0][1], keep[1][1], keep[2][1], tab.data_ptr(), len(side) if I is None else I, S,
                     out.data_ptr(), None)


def test_every_refusal_raises_by_name():
    p = torch.rand(10, 3, device=DEV)
    for S in (0, 4097):
        with pytest.raises(ValueError, match=r"gn_render_points_batch: image size S=%d outside \[1, 4096\]" % S):
            ops.render_points_batch(p, [0, 10], ["front"], [1], S)
        with pytest.raises(ValueError, match=r"gn_render_points_batch: image size S=%d outside \[1, 4096\]" % S):
            _entry([0, 10], [0], [1], S)
        with pytest.raises(ValueError, match=r"gn_color_idx_batch: image size S=%d outside" % S):
            _lib.call("gn_color_idx_batch", None, None, None, None, None, 1, S, None, None)
    for k in (0, 9):
        with pytest.raises(ValueError, match=r"gn_render_points_batch: image 1: kernel_size k=%d outside \[1, S=8\]" % k):
            ops.render_points_batch(p, [0, 5, 10], ["front", "top"], [8, k], 8)
    with pytest.raises(ValueError, match=r"gn_render_points_batch: I=65536 images outside \[0, 65535\]"):
        ops.render_points_batch(p, [0] * 65537, ["front"] * 65536, [1] * 65536, 1)
    with pytest.raises(ValueError, match=r"gn_render_points_batch: I=65536 images outside \[0, 65535\]"):
        _entry([0, 0], [0], [1], 8, I=65536)
    with pytest.raises(ValueError, match=r"gn_render_points_batch: image 0: a segment of 4294967295 points \(needs fewer than 2\^32 - 1\)"):
        _entry([0, 2 ** 32 - 1], [0], [1], 8)
    with pytest.raises(ValueError, match="seg must be non-decreasing"):
        ops.render_points_batch(p, [0, 6, 5, 10], ["front"] * 3, [1] * 3, 8)
    with pytest.raises(ValueError, match="seg must be non-decreasing"):
        ops.render_points_batch(p, [0, 11], ["front"], [1], 8)
    with pytest.raises(ValueError, match=r"gn_render_points_batch: image 0: seg is not a non-decreasing CSR"):
        _entry([5, 3], [0], [1], 8)
    for side in (3, -1):
        with pytest.raises(ValueError, match=r"gn_render_points_batch: image 0: side=%d outside" % side):
            ops.render_points_batch(p, [0, 10], [side], [1], 8)
    with pytest.raises(TypeError):
        ops.render_points_batch(p.double(), [0, 10], ["front"], [1], 8)
    idx = ops.render_points_batch(p, [0, 10], ["front"], [2], 8)
    over = ((0.5, 0.5, 0.5), (1, 0, 0, 1), 4)
    with pytest.raises(ValueError, match="4 overlays"):
        ops.color_idx_batch(idx, [{"count": 10, "overlays": [over] * 4}], colors=torch.rand(10, 4, device=DEV))
    for k in (0, 9):
        with pytest.raises(ValueError, match=r"gn_color_idx_batch: image 0: overlay 1: kernel_size k=%d outside \[1, S=8\]" % k):
            ops.color_idx_batch(idx, [{"count": 10, "overlays": [over, (over[0], over[1], k)]}], colors=torch.rand(10, 4, device=DEV))
    with pytest.raises(ValueError, match=r"gn_color_idx_batch: image 0: side=5 outside"):
        ops.color_idx_batch(idx, [{"count": 10, "side": 5}], colors=torch.rand(10, 4, device=DEV))
    with pytest.raises(ValueError, match="unknown mode"):
        ops.color_idx_batch(idx, [{"count": 10, "mode": "jet"}], colors=torch.rand(10, 4, device=DEV))
    with pytest.raises(ValueError, match="outside the image's colour source"):
        ops.color_idx_batch(idx, [{"count": 11}], colors=torch.rand(10, 4, device=DEV))
    with pytest.raises(_lib.GarmentNetsHipError, match="no CPU fallback"):
        ops.render_points_batch(p.cpu(), [0, 10], ["front"], [1], 8)


# ------------------------------------------------------------------------------------------------ 4. both training loops
FLAGS = ["--vis_per_items", "1", "--max_vis_per_epoch_train", "2", "--max_vis_per_epoch_val", "2"]
NAMES = ["train_0.png", "train_1.png", "val_0.png", "val_1.png"]       # batches of 2: the first batch of each loop fills the limit of 2


def _same_state(a, b):
    a, b = a.state_dict(), b.state_dict()
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def _run_with_and_without(main, common, tmp_path, monkeypatch, shape):
    """common carries --static_epoch_seed: without it the train subset draws its points from OS entropy and no two runs see the same batches"""
    plain = main(common + ["--output_dir", str(tmp_path / "plain")])
    assert not (tmp_path / "plain" / "vis").exists()
    calls = []
    render = V.render_batch
    monkeypatch.setattr(V, "render_batch", lambda specs, img_size=256, backend="device", device=None:
                        calls.append((list(specs), img_size)) or render(specs, img_size, backend, device))
    drawn = main(common + ["--output_dir", str(tmp_path / "drawn")] + FLAGS)
    folder = tmp_path / "drawn" / "vis" / "epoch_000"
    assert sorted(os.listdir(tmp_path / "drawn" / "vis")) == ["epoch_000"] and sorted(os.listdir(folder)) == NAMES
    images = {name: V.read_png(str(folder / name)) for name in NAMES}
    assert all(img.shape == shape and img.dtype == np.uint8 for img in images.values())
    assert len(calls) == 2 and all(img_size == 256 for _, img_size in calls)        # one render per loop: the later batches select nobody
    for (specs, _), prefix in zip(calls, ("train_", "val_")):                       # the step's own tensors through the numpy backend
        restated = V.compose(render(specs, 256, "numpy"), len(specs) // 2)
        for j, img in enumerate(restated):
            assert img.shape == shape and np.array_equal(V.to_uint8(img), images["%s%d.png" % (prefix, j)]), (prefix, j)
    assert any(np.any(img[..., 3] > 0) for img in images.values())
    assert _same_state(plain["model"], drawn["model"])                               # the monitors do not move training
    assert drawn["model"].hparams["vis_per_items"] == 1 and plain["model"].hparams["vis_per_items"] == 0
    return drawn


def test_first_stage_training_writes_its_monitors(tmp_path, monkeypatch):
    from garmentnets_amd import train as T
    from test_validate_host import write_validation_store
    store = tmp_path / "ds.zarr"
    write_validation_store(str(store), 20)
    common = ["--model", "pointnet2", "--zarr_in", str(store), "--epochs", "1", "--num_batches", "2", "--batch_size", "2", "--num_pc_sample", "400",
              "--static_epoch_seed"]
    # the NOCS pair above the confidence pair (the synthetic head has bins): two rows of two 256 x 256 images
    _run_with_and_without(T.main, common, tmp_path, monkeypatch, (512, 512, 4))


def test_second_stage_training_writes_its_monitors(tmp_path, monkeypatch):
    from garmentnets_amd import train_pipeline as TP
    from test_validate_host import VOLUME_SIZE, write_validation_store
    store = tmp_path / "ds.zarr"
    write_validation_store(str(store), 20)
    common = ["--zarr_in", str(store), "--volume_size", str(VOLUME_SIZE), "--epochs", "1", "--num_batches", "2", "--batch_size", "2",
              "--num_pc_sample", "400", "--num_volume_sample", "96", "--num_surface_sample", "80", "--grid", "8", "--static_epoch_seed"]
    # the NOCS pair above the pair of WNF slices
    _run_with_and_without(TP.main, common, tmp_path, monkeypatch, (512, 512, 4))
