#!/usr/bin/env python3
"""Golden images for the training monitors from the REFERENCE's own renderer (build container only).

Run:  python tests/golden/make_golden_render.py        (needs the reference and matplotlib; never runs on the GPU box)

The reference's common/rendering_util.py and common/visualization_util.py are imported as they are, with three stand-ins for what is absent here:
numba.jit becomes a pass-through decorator factory (the splat then runs as the plain Python loop it is, its uint32 pixels widened to int64 as numba's
typing widens them), skimage.transform is an empty stub (only render_wnf reads it, which nothing here calls), and matplotlib.cm.get_cmap -- removed
in matplotlib 3.9 -- is matplotlib.colormaps[name].
Only DATA (seeded inputs, the images the reference makes of them) is written to tests/golden/ref_render.npz.

Every finite point keeps its camera coordinates c within c * (S - 1) > -1 and c <= 1.5 (asserted), where the reference's uint32 cast is the same on
every platform.  Keys: <case>/<field>; tests/render_cases.py turns every case into the matching call of garmentnets_amd.visualize.
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ref as G  # noqa: E402

S = 32
SIDES = ("front", "top", "left")
KERNELS = (1, 4, 5, 8)
VIS_ARGS = [(0, 4, 4, 1, 3), (1, 4, 4, 1, 6), (2, 4, 3, 2, 10), (3, 24, 7, 5, 100), (0, 2, 2, 1, 0), (5, 3, 1, 4, 4)]


def load_reference():
    import matplotlib
    import matplotlib.cm
    numba = types.ModuleType("numba")
    # numba types `uint32 pixel + int64 offset` as int64; plain numpy scalars refuse a negative offset on a uint32, so the loop gets its pixels as int64
    numba.jit = lambda *a, **k: (lambda f: (lambda xy_idx, *rest: f(xy_idx.astype(np.int64), *rest)))
    skimage = types.ModuleType("skimage")
    skimage.transform = types.ModuleType("skimage.transform")
    skimage.transform.resize = None
    sys.modules.update({"numba": numba, "skimage": skimage, "skimage.transform": skimage.transform})
    if not hasattr(matplotlib.cm, "get_cmap"):
        matplotlib.cm.get_cmap = lambda name: matplotlib.colormaps[name]
    sys.path.insert(0, G.REF)
    from common import rendering_util as R, visualization_util as V
    return R, V


def check_range(R, points, side, size):
    p = points[np.isfinite(points).all(axis=1)]
    c = R.to_camera(p, R.get_extrinsic(side))[:, :2]
    assert np.all(c * (size - 1) > -1) and np.all(c <= 1.5), "a camera coordinate leaves the platform-independent range"


def cloud(rng):
    """300 random points, the first 20 again (equal depths), every corner / edge / face centre of the unit cube, and a few just outside it"""
    p = rng.rand(300, 3).astype(np.float32)
    grid = np.stack(np.meshgrid(*[[0.0, 0.5, 1.0]] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    outside = np.array([[-0.02, 0.5, 0.5], [1.3, 0.2, 0.7], [0.4, -0.02, 1.02], [0.6, 1.02, -0.03], [1.02, 1.03, 0.1]], dtype=np.float32)
    return np.concatenate([p, p[:20], grid, outside, grid[::-1]])


def main():
    assert os.path.isdir(G.REF), "reference not mounted: goldens can only be generated in the build container"
    R, V = load_reference()
    rng = np.random.RandomState(20240611)
    out = {}

    def nocs_case(name, points, side, k, size=S):
        check_range(R, points, side, size)
        out[name + "/points"], out[name + "/side"], out[name + "/k"], out[name + "/S"] = points, np.array(side), np.int64(k), np.int64(size)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)            # (the cast of a NaN pixel of a point that is never drawn)
            idx = R.render_points_idx(R.to_camera(points, R.get_extrinsic(side)), img_size=size, kernel_size=k)
            img = R.render_nocs(points, side=side, img_size=size, kernel_size=k)
        assert idx.dtype == np.uint32 and img.dtype == np.float32
        return idx, img

    pts = cloud(rng)
    for side in SIDES:
        for k in KERNELS:
            name = f"cloud_{side}_k{k}"
            out[name + "/idx"], out[name + "/img"] = nocs_case(name, pts, side, k)

    bad = rng.rand(100, 3).astype(np.float32)
    bad[3, 0], bad[10, 0], bad[17, 2], bad[25, 2] = np.nan, np.inf, np.nan, np.inf
    bad[31, 1], bad[40, 0], bad[47, 2] = np.inf, -np.inf, -np.inf
    out["nonfinite/idx"], out["nonfinite/img"] = nocs_case("nonfinite", bad, "front", 4)
    for i in (3, 10, 17, 25, 31, 40, 47):
        assert not np.any(out["nonfinite/idx"] == i)
    out["empty/idx"], out["empty/img"] = nocs_case("empty", np.zeros((0, 3), np.float32), "front", 4)

    big = rng.rand(6000, 3).astype(np.float32)
    idx, img = nocs_case("big", big, "front", 4, size=256)
    out["big/idx"], out["big/img_sub"] = idx, img[::8, ::8].copy()

    # WNF slices: the special values sit on queries inside the slice, apart from each other and nearest to the camera (depth = y)
    q = rng.rand(600, 3).astype(np.float32)
    wnf = (rng.rand(600) * 2.4 - 0.7).astype(np.float32)
    special = [(-0.8, 0.1, 0.1), (1.9, 0.5, 0.1), (1.5, 0.9, 0.1), (np.nan, 0.1, 0.9), (-0.5, 0.5, 0.9), (1.4999999, 0.9, 0.9), (np.inf, 0.5, 0.5),
               (-np.inf, 0.1, 0.5)]
    for j, (v, x, z) in enumerate(special):
        q[j], wnf[j] = (x, 0.5001 + 1e-4 * j, z), v
    check_range(R, q, "front", S)
    out["wnf/query"], out["wnf/values"] = q, wnf
    out["wnf/img"] = R.render_wnf_points(q, wnf, img_size=S).astype(np.float32)
    assert out["wnf/img"].shape == (S, S, 4)
    pred = (wnf + rng.randn(600).astype(np.float32) * np.float32(0.2)).astype(np.float32)
    out["wnf_pair/pred"] = pred
    out["wnf_pair/img"] = V.render_wnf_points_pair(q, wnf, pred, img_size=S)
    q_none = q.copy()
    q_none[:, 1] = np.where(q_none[:, 1] < 0.55, 0.5, 0.6).astype(np.float32)        # on the open interval's ends: nothing is selected
    out["wnf_none/query"] = q_none
    out["wnf_none/img"] = R.render_wnf_points(q_none, wnf, img_size=S)

    # a NOCS pair with its three grip points, and the confidence images (render_confidence_pair's two halves at this size: the pair itself
    # ignores its img_size)
    gt = rng.rand(500, 3).astype(np.float32)
    pr = np.clip(gt + rng.randn(500, 3).astype(np.float32) * np.float32(0.05), 0, 1).astype(np.float32)
    grips = np.array([[0.5, 0.3, 0.98], [0.02, 0.6, 0.5], [0.93, 0.1, 0.04]], dtype=np.float32)
    conf = rng.rand(500).astype(np.float32)
    conf[:4] = [0.0, 1.0, 0.999, np.float32(1.0) - np.float32(2.0 ** -24)]
    for a in (gt, pr, grips):
        check_range(R, a, "front", S)
    out["pair/gt"], out["pair/pred"], out["pair/grips"], out["pair/confidence"] = gt, pr, grips, conf
    out["pair/img"] = V.render_nocs_pair(gt, pr, grips[0], grips[1], grips[2], img_size=S, kernel_size=4)
    out["pair/img_two_grips"] = V.render_nocs_pair(gt, pr, grips[0], grips[1], img_size=S, kernel_size=5)
    out["pair/confidence_img"] = np.concatenate([R.render_points_confidence(gt, conf, img_size=S), R.render_points_confidence(pr, conf, img_size=S)], axis=1)
    out["pair/overlay_img"] = V.overlay_grip(out["cloud_front_k4/img"], grips[0], color=(0, 1, 0, 1), kernel_size=8)

    out["vis/args"] = np.array(VIS_ARGS, dtype=np.int64)
    for j, (batch_idx, batch_size, this, per, limit) in enumerate(VIS_ARGS):
        res = V.get_vis_idxs(batch_idx, batch_size=batch_size, this_batch_size=this, vis_per_items=per, max_vis_per_epoch=limit)
        for key, val in zip(("global", "selected", "vis"), res):
            out[f"vis/{j}/{key}"] = np.array(val, dtype=np.int64)

    for k, v in out.items():
        assert isinstance(v, np.ndarray) or np.isscalar(v), k
    path = os.path.join(HERE, "ref_render.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
