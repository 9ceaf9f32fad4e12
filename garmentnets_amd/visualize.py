"""The training monitors: the image pairs the reference's vis_batch logs (common/rendering_util.py, common/visualization_util.py), by its names --
render_points_idx, render_nocs, render_nocs_pair, render_confidence_pair, render_wnf_points, render_wnf_points_pair, overlay_grip, get_vis_idxs -- and
write_png / read_png for them.

Every image is described by one `image_spec` (points, side, footprint, a colour table or scalars through viridis, overlay points) and rendered by
`render_batch`, which has two backends held to the same definitions ("Training monitors"):

  backend="device"   all images of the call in ONE launch pair: ops.render_points_batch (the z-buffered splat, csrc/render.hip) and ops.color_idx_batch.
                     The inputs are torch tensors on the device (numpy arrays are uploaded to the current device); the images' point sets travel as
                     one concatenated tensor with a CSR, and only the finished images come back to the host.  The default.
  backend="numpy"    the restatement on the host, written from the definitions: the vectorised winner rule (every covered pixel of every point, the
                     smallest fp64 depth per pixel, the lowest index among equal depths) -- not a port of the reference's serial loop.

Differences from the reference, all outside what its training calls do: points are fp32 (they are cast); the camera is one of the three get_extrinsic
sides and sits INSIDE render_points_idx (the reference's takes camera coordinates); a camera coordinate with c * (S - 1) <= -1 clamps to pixel 0 (the
reference's uint32 cast wraps there); a point with any non-finite coordinate is not drawn; render_confidence_pair honours its img_size / kernel_size
(the reference ignores them and renders 256 / 4, which are the defaults here).  render_wnf / render_wnf_pair (skimage's resize; never called in
training) are not provided.

Mesh images (the evaluation's visualisation; DESIGN.md, "Mesh images") are described by `mesh_spec` (vertices, faces, a colour row per vertex, side,
ambient) and rendered by `render_mesh_batch`, again on the device (ops.render_mesh_batch + ops.color_mesh_batch, one launch pair for all of them) or
by the numpy restatement: a z-buffered, two-sided, shaded triangle rasteriser whose coverage is decided in integers.  The coverage rules, the drawn
faces, the index image and the winner's weights live in raster.py, shared with point_cloud.py; this module brings its axis cameras, the depth, the
colour mix and the shade.
"""
import os
import re
import struct
import zlib

import numpy as np

from . import raster
from .raster import DEFAULT_IDX, MESH_COORD_LIMIT, MESH_SUBPIXEL, _host  # noqa: F401  (the constants are this module's public names too)

# side -> per camera coordinate (axis of the point, sign, offset): the reference's get_extrinsic, each row one signed unit vector plus a translation
SIDES = {"front": ((0, 1.0, 0.0), (2, -1.0, 1.0), (1, 1.0, 0.0)),
         "top": ((0, 1.0, 0.0), (1, -1.0, 1.0), (2, -1.0, 1.0)),
         "left": ((1, -1.0, 1.0), (2, -1.0, 1.0), (0, 1.0, 0.0))}
WNF_RANGE, CONFIDENCE_RANGE = (-0.5, 1.5), (0.0, 1.0)
_LUT = None


def viridis_lut():
    """float32(matplotlib's viridis.colors) with alpha 1, (256, 4): the table of csrc/viridis_lut.h (tools/gen_viridis_lut.py), which the colour kernel
    compiles in; matplotlib is not needed"""
    global _LUT
    if _LUT is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "viridis_lut.h")) as f:
            bits = np.array([int(t, 16) for t in re.findall(r"0x([0-9a-f]{8})u", f.read())], dtype=np.uint32)
        if bits.shape[0] != 768:
            raise ValueError(f"csrc/viridis_lut.h: expected 768 entries, found {bits.shape[0]}")
        _LUT = np.concatenate([bits.view(np.float32).reshape(256, 3), np.ones((256, 1), np.float32)], axis=1)
    return _LUT


# ------------------------------------------------------------------------------------------------ the numpy restatement
def to_camera(points, side="front"):
    """(N, 3) fp32 -> (N, 3) fp64 camera coordinates: cam[j] = sign_j * double(p[axis_j]) + t_j, one rounding per coordinate"""
    p = _host(points).reshape(-1, 3).astype(np.float64)
    return np.stack([sign * p[:, axis] + t for axis, sign, t in SIDES[side]], axis=1)


def _pixels(c, S):
    """clamp(trunc(c * (S - 1)), 0, S - 1) in fp64, for finite c"""
    return np.clip(np.trunc(c * np.float64(S - 1)), 0, S - 1).astype(np.int64)


def _render_points_idx_numpy(points, side, S, k):
    p = _host(points).reshape(-1, 3)
    img = np.full((S, S), DEFAULT_IDX, dtype=np.uint32)
    cam = to_camera(p, side)
    drawn = np.flatnonzero(np.isfinite(p).all(axis=1) & (cam[:, 2] < np.inf))          # +inf and NaN depths never win
    if drawn.size == 0:
        return img
    x, y, z = _pixels(cam[drawn, 0], S), _pixels(cam[drawn, 1], S), cam[drawn, 2]
    d = np.arange(k, dtype=np.int64) - k // 2                                           # the footprint's offsets
    X = np.broadcast_to(x[:, None, None] + d[None, None, :], (x.size, k, k))
    Y = np.broadcast_to(y[:, None, None] + d[None, :, None], (x.size, k, k))
    inside = (X >= 0) & (X <= S - 1) & (Y >= 0) & (Y <= S - 1)
    pixel = (Y * S + X)[inside]
    depth = np.broadcast_to(z[:, None, None], X.shape)[inside]
    index = np.broadcast_to(drawn[:, None, None], X.shape)[inside]
    order = np.lexsort((index, depth, pixel))                                           # per pixel: the smallest depth, then the lowest index
    first = np.ones(order.size, dtype=bool)
    first[1:] = pixel[order][1:] != pixel[order][:-1]
    img.reshape(-1)[pixel[order][first]] = index[order][first].astype(np.uint32)
    return img


def viridis(x, vmin, vmax):
    """matplotlib's Colormap.__call__ of viridis on fp32 values -> (N, 4) fp32: v = (x - vmin) / (vmax - vmin) and u = v * 256 in fp32; entry trunc(u),
    u == 256 -> 255, under -> 0, over -> 255, NaN -> (0, 0, 0, 0)"""
    x = _host(x).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x - np.float32(vmin)) / (np.float32(vmax) - np.float32(vmin)) * np.float32(256)
        e = np.where(u < 0, 0, np.where(u >= 256, 255, np.trunc(np.where(np.isnan(u), 0, u)))).astype(np.int64)
    out = viridis_lut()[e]
    out[np.isnan(u)] = 0
    return out


def color_idx_img(idx_img, colors, default_color=(1, 1, 1)):
    """the reference's color_idx_img: fp32, default_color where the index is 0xFFFFFFFF, else colors[idx]"""
    default_color = np.asarray(default_color, dtype=np.float32)
    img = np.empty(idx_img.shape + (len(default_color),), dtype=np.float32)
    img[:, :] = default_color
    drawn = idx_img != DEFAULT_IDX
    img[drawn] = np.asarray(colors)[idx_img[drawn]].astype(np.float32)
    return img


def _render_spec_numpy(spec, S):
    idx = _render_points_idx_numpy(spec["points"], spec["side"], S, spec["kernel_size"])
    colors = _host(spec["colors"]).reshape(-1, 4) if spec["values"] is None else viridis(spec["values"], *spec["vrange"])
    img = color_idx_img(idx, colors, spec["default_color"])
    for xyz, rgba, k in spec["overlays"]:                                               # overlay_grip: a one-point image, copied where its alpha > 0
        one = color_idx_img(_render_points_idx_numpy(np.asarray(xyz, np.float32)[None], spec["side"], S, k), np.asarray([rgba], np.float32), (1, 1, 1, 0))
        is_grip = one[:, :, 3] > 0
        img[is_grip] = one[is_grip]
    return img


# ------------------------------------------------------------------------------------------------ image specs and the two backends
def image_spec(points, side="front", kernel_size=4, colors=None, values=None, vrange=None, default_color=(1, 1, 1, 0), overlays=()):
    """one image: (N, 3) points seen from `side` with a kernel_size-wide footprint, coloured by `colors` ((N, 4) RGBA; None with no values: the points
    themselves with alpha 1) or by `values` ((N,) scalars through viridis over vrange = (min, max)); overlays: up to three (xyz, rgba, kernel_size),
    applied in order.  points / colors / values: numpy arrays or torch tensors"""
    if side not in SIDES:
        raise ValueError(f"side={side!r}: expected one of {tuple(SIDES)}")
    if values is not None and (colors is not None or vrange is None):
        raise ValueError("image_spec: values come with vrange and without colors")
    if any(src is not None and len(src) != len(points) for src in (colors, values)):
        raise ValueError(f"image_spec: one colour row / value per point ({len(points)} points)")
    overlays = [(xyz, tuple(float(v) for v in rgba), int(k)) for xyz, rgba, k in overlays]
    return {"points": points, "side": side, "kernel_size": int(kernel_size), "colors": colors, "values": values, "vrange": vrange,
            "default_color": tuple(float(v) for v in default_color), "overlays": overlays}


def _check_spec(spec, S):
    if len(spec["default_color"]) != 4:
        raise ValueError("default_color: expected 4 floats (RGBA)")
    if not 1 <= spec["kernel_size"] <= S or any(not 1 <= k <= S for _, _, k in spec["overlays"]):
        raise ValueError(f"kernel_size outside [1, S={S}]")


def _render_batch_numpy(specs, S):
    out = np.empty((len(specs), S, S, 4), dtype=np.float32)
    for i, spec in enumerate(specs):
        p = _host(spec["points"]).reshape(-1, 3)
        colors = spec["colors"]
        if colors is None and spec["values"] is None:                                   # the reference's [points, 1]
            colors = np.concatenate([p, np.ones((len(p), 1), np.float32)], axis=1)
        out[i] = _render_spec_numpy(dict(spec, points=p, colors=colors, overlays=[(_host(xyz).reshape(3), c, k) for xyz, c, k in spec["overlays"]]), S)
    return out


class _Rows:
    """tensors laid back to back; one that several images read (a NOCS pair's colours) is stored once"""

    def __init__(self):
        self.tensors, self.first, self.n = [], {}, 0

    def add(self, key, make):
        if key not in self.first:
            t = make()
            self.first[key] = self.n
            self.n += t.shape[0]
            self.tensors.append(t)
        return self.first[key]

    def joint(self):
        import torch
        return None if not self.tensors else (torch.cat(self.tensors) if len(self.tensors) > 1 else self.tensors[0]).contiguous()


def _render_batch_device(specs, S, device=None):
    import torch

    from . import ops

    def dev(a, width):
        if not torch.is_tensor(a):
            a = torch.from_numpy(_host(a)).to(device or "cuda")
        a = a.detach().to(torch.float32)
        return a.reshape(-1, width) if width else a.reshape(-1)

    if not specs:
        return np.empty((0, S, S, 4), dtype=np.float32)
    points = [dev(s["points"], 3) for s in specs]
    seg = np.concatenate([[0], np.cumsum([p.shape[0] for p in points])])
    grips = [xyz for s in specs for xyz, _, _ in s["overlays"]]                         # every overlay point of the call in one copy to the host
    down = [g for g in grips if torch.is_tensor(g)]
    down = iter(torch.stack([dev(g, 0) for g in down]).cpu().tolist() if down else ())
    grips = iter([next(down) if torch.is_tensor(g) else _host(g).reshape(3).tolist() for g in grips])
    tables = {"colors": _Rows(), "values": _Rows()}
    images = []
    for spec, p in zip(specs, points):
        key = "colors" if spec["values"] is None else "values"
        src = spec[key]
        if src is None:
            first = tables[key].add(("points", id(spec["points"])), lambda: torch.cat([p, p.new_ones((p.shape[0], 1))], dim=1))
        else:
            first = tables[key].add(id(src), lambda: dev(src, 4 if key == "colors" else 0))
        vmin, vmax = spec["vrange"] or (0.0, 1.0)
        images.append({"offset": first, "count": p.shape[0], "mode": "table" if key == "colors" else "viridis", "side": spec["side"], "vmin": vmin,
                       "vmax": vmax, "default_color": spec["default_color"], "overlays": [(next(grips), c, k) for _, c, k in spec["overlays"]]})
    idx = ops.render_points_batch((torch.cat(points) if len(points) > 1 else points[0]).contiguous(), seg, [s["side"] for s in specs],
                                  [s["kernel_size"] for s in specs], S)
    return ops.color_idx_batch(idx, images, colors=tables["colors"].joint(), values=tables["values"].joint()).cpu().numpy()


def render_batch(specs, img_size=256, backend="device", device=None):
    """every image of `specs` (image_spec) -> (I, S, S, 4) fp32 on the host.  backend "device": one launch pair for all of them; "numpy": the restatement"""
    specs = list(specs)
    S = int(img_size)
    if backend not in ("device", "numpy"):
        raise ValueError(f"backend={backend!r}: expected 'device' or 'numpy'")
    for spec in specs:
        _check_spec(spec, S)
    return _render_batch_numpy(specs, S) if backend == "numpy" else _render_batch_device(specs, S, device)


def render_idx_batch(points, sides, kernel_sizes, img_size=256, backend="device", device=None):
    """the index images alone: points[i] seen from sides[i] under kernel_sizes[i] -> (I, S, S) uint32 on the host"""
    S = int(img_size)
    if backend == "numpy":
        return np.stack([_render_points_idx_numpy(p, s, S, int(k)) for p, s, k in zip(points, sides, kernel_sizes)]) if len(points) else \
            np.empty((0, S, S), np.uint32)
    import torch

    from . import ops
    pts = [(p if torch.is_tensor(p) else torch.from_numpy(_host(p)).to(device or "cuda")).detach().to(torch.float32).reshape(-1, 3) for p in points]
    seg = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])]).astype(np.int64)
    joint = torch.cat(pts).contiguous() if pts else torch.empty((0, 3), dtype=torch.float32, device=device or "cuda")
    return ops.render_points_batch(joint, seg, sides, kernel_sizes, S).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ mesh images
# DESIGN.md "Mesh images": a z-buffered, two-sided, shaded triangle rasteriser behind the same camera.  Coverage is decided in integers on 1/256-pixel
# fixed-point coordinates (raster.py), so the numpy restatement below and csrc/render.hip agree bit for bit.
DEFAULT_AMBIENT = 0.35                          # a look, not a measurement: how dark a face seen edge-on gets


def _mesh_faces(verts, faces, side, S):
    """raster.drawn_faces behind the axis camera of `side`: screen = cam * (S - 1), nothing culled"""
    def project(v):
        cam = to_camera(v, side)
        return cam, cam[:, 0] * np.float64(S - 1), cam[:, 1] * np.float64(S - 1), np.ones(len(v), dtype=bool)
    return raster.drawn_faces(verts, faces, project)


def _render_mesh_idx_numpy(verts, faces, side, S):
    return _render_mesh_numpy(verts, faces, side, S)[0]


def _render_mesh_numpy(verts, faces, side, S):
    """-> (index image (S, S) uint32, the winners' depths (S, S) fp64, +inf where nobody covers)"""
    index, _, fx, fy, cam = _mesh_faces(verts, faces, side, S)

    def depth(face, wa, wb, wc):
        z = cam[face][:, :, 2]
        return ((wa.astype(np.float64) * z[:, 0] + wb.astype(np.float64) * z[:, 1]) + wc.astype(np.float64) * z[:, 2]) / (wa + wb + wc).astype(np.float64)
    return raster.raster_idx(index, fx, fy, S, depth, largest=False)


def _color_mesh_numpy(idx_img, verts, faces, colors, side, ambient, default_color):
    S = idx_img.shape[0]
    img = np.empty((S, S, 4), dtype=np.float32)
    img[:, :] = np.asarray(default_color, dtype=np.float32)
    index, f, fx, fy, cam = _mesh_faces(verts, faces, side, S)
    Y, X, row, wa, wb, wc = raster.winner_weights(idx_img, index, fx, fy)
    if len(Y) == 0:
        return img
    area2 = (wa + wb + wc).astype(np.float64)
    beta = [(w.astype(np.float64) / area2).astype(np.float32) for w in (wa, wb, wc)]
    c = _host(colors).reshape(-1, 4)[f[row]]                                            # (P, 3 corners, 4)
    rgb = (beta[0][:, None] * c[:, 0, :3] + beta[1][:, None] * c[:, 1, :3]) + beta[2][:, None] * c[:, 2, :3]
    nx, ny, nz = raster.face_normals(cam[row])
    amb = np.float64(np.float32(ambient))
    with np.errstate(all="ignore"):
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        shade = np.where((length > 0) & np.isfinite(length), amb + (1.0 - amb) * (np.abs(nz) / length), amb)
    img[Y, X, :3] = shade.astype(np.float32)[:, None] * rgb
    img[Y, X, 3] = 1
    return img


def mesh_spec(verts, faces, colors, side="front", ambient=DEFAULT_AMBIENT, default_color=(1, 1, 1, 0)):
    """one mesh image: (V, 3) vertices and (F, 3) faces seen from `side`, coloured per vertex by `colors` ((V, 4) RGBA; scalar colourings are built
    with `viridis`), shaded by ambient + (1 - ambient) * |n_z| / |n|.  verts / faces / colors: numpy arrays or torch tensors"""
    if side not in SIDES:
        raise ValueError(f"side={side!r}: expected one of {tuple(SIDES)}")
    if len(colors) != len(verts):
        raise ValueError(f"mesh_spec: one colour row per vertex ({len(verts)} vertices, {len(colors)} rows)")
    if len(default_color) != 4:
        raise ValueError("default_color: expected 4 floats (RGBA)")
    return {"verts": verts, "faces": faces, "colors": colors, "side": side, "ambient": float(ambient),
            "default_color": tuple(float(v) for v in default_color)}


def _mesh_device_args(specs, device):
    from . import ops
    return ops.pack_meshes([(s["verts"], s["faces"], s["colors"]) for s in specs], (4,), device)


def render_mesh_idx_batch(specs, img_size=256, backend="device", device=None):
    """the index images alone -> (I, S, S) uint32 on the host: per pixel the face (counted within its image) that covers the pixel's sample nearest
    to the camera, 0xFFFFFFFF where there is none"""
    specs, S = list(specs), int(img_size)
    if backend not in ("device", "numpy"):
        raise ValueError(f"backend={backend!r}: expected 'device' or 'numpy'")
    if not specs:
        return np.empty((0, S, S), np.uint32)
    if backend == "numpy":
        return np.stack([_render_mesh_idx_numpy(s["verts"], s["faces"], s["side"], S) for s in specs])
    from . import ops
    verts, faces, _, vseg, fseg = _mesh_device_args(specs, device)
    return ops.render_mesh_batch(verts, faces, vseg, fseg, [s["side"] for s in specs], S).cpu().numpy().view(np.uint32)


def render_mesh_batch(specs, img_size=256, backend="device", device=None):
    """every mesh image of `specs` (mesh_spec) -> (I, S, S, 4) fp32 on the host.  backend "device": one launch pair (ops.render_mesh_batch,
    ops.color_mesh_batch) for all of them; "numpy": the restatement"""
    specs, S = list(specs), int(img_size)
    if backend not in ("device", "numpy"):
        raise ValueError(f"backend={backend!r}: expected 'device' or 'numpy'")
    if not specs:
        return np.empty((0, S, S, 4), dtype=np.float32)
    if backend == "numpy":
        return np.stack([_color_mesh_numpy(_render_mesh_idx_numpy(s["verts"], s["faces"], s["side"], S), s["verts"], s["faces"], s["colors"],
                                           s["side"], s["ambient"], s["default_color"]) for s in specs])
    from . import ops
    verts, faces, colors, vseg, fseg = _mesh_device_args(specs, device)
    sides = [s["side"] for s in specs]
    idx = ops.render_mesh_batch(verts, faces, vseg, fseg, sides, S)
    return ops.color_mesh_batch(idx, verts, faces, colors, vseg, fseg, sides, [s["ambient"] for s in specs],
                                [s["default_color"] for s in specs]).cpu().numpy()


# ------------------------------------------------------------------------------------------------ the reference's API
def render_points_idx(points, img_size=256, kernel_size=4, side="front", backend="device"):
    """-> (S, S) uint32: per pixel the index of the covering point nearest to the camera of `side`, 0xFFFFFFFF where there is none"""
    return render_idx_batch([points], [side], [kernel_size], img_size, backend)[0]


def render_nocs(points, colors=None, side="front", img_size=256, kernel_size=4, default_color=(1, 1, 1, 0), backend="device"):
    return render_batch([image_spec(points, side, kernel_size, colors=colors, default_color=default_color)], img_size, backend)[0]


def overlay_grip(img, grip_nocs, color=(1, 0, 0, 1), side="front", kernel_size=4, backend="device"):
    """a copy of the (S, S, 4) image with the one-point image of grip_nocs over it where that one's alpha > 0"""
    assert img.shape[0] == img.shape[1]
    grip_img = render_batch([image_spec(_host(grip_nocs).reshape(1, 3), side, kernel_size, colors=np.asarray([color], np.float32))], img.shape[0], backend)[0]
    is_grip = grip_img[:, :, 3] > 0
    new_img = img.copy()
    new_img[is_grip] = grip_img[is_grip]
    return new_img


def nocs_pair_specs(gt_nocs, pred_nocs, gt_grip_nocs=None, pred_grip_nocs=None, pred_grip_nocs_nn=None, side="front", kernel_size=4):
    """the two images of render_nocs_pair: both coloured [gt_nocs, 1]; ground-truth red on the first, predicted red then nearest-point green on the second"""
    red, green = (1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0)
    colors = _nocs_colors(gt_nocs)
    gt_over = [] if gt_grip_nocs is None else [(gt_grip_nocs, red, kernel_size * 2)]
    pred_over = ([] if pred_grip_nocs is None else [(pred_grip_nocs, red, kernel_size * 2)]) + \
        ([] if pred_grip_nocs_nn is None else [(pred_grip_nocs_nn, green, kernel_size * 2)])
    return [image_spec(gt_nocs, side, kernel_size, colors=colors, overlays=gt_over), image_spec(pred_nocs, side, kernel_size, colors=colors, overlays=pred_over)]


def _nocs_colors(gt_nocs):
    if hasattr(gt_nocs, "detach"):
        import torch
        g = gt_nocs.detach().to(torch.float32).reshape(-1, 3)
        return torch.cat([g, g.new_ones((g.shape[0], 1))], dim=1)
    g = _host(gt_nocs).reshape(-1, 3)
    return np.concatenate([g, np.ones((len(g), 1), np.float32)], axis=1)


def scalar_pair_specs(points_a, points_b, values_a, values_b, vrange, side="front", kernel_size=4):
    return [image_spec(points_a, side, kernel_size, values=values_a, vrange=vrange), image_spec(points_b, side, kernel_size, values=values_b, vrange=vrange)]


def _pair(imgs):
    return np.concatenate([imgs[0], imgs[1]], axis=1)


def render_nocs_pair(gt_nocs, pred_nocs, gt_grip_nocs=None, pred_grip_nocs=None, pred_grip_nocs_nn=None, side="front", img_size=256, kernel_size=4,
                     backend="device"):
    return _pair(render_batch(nocs_pair_specs(gt_nocs, pred_nocs, gt_grip_nocs, pred_grip_nocs, pred_grip_nocs_nn, side, kernel_size), img_size, backend))


def render_confidence_pair(gt_nocs, pred_nocs, confidence, side="front", img_size=256, kernel_size=4, backend="device"):
    return _pair(render_batch(scalar_pair_specs(gt_nocs, pred_nocs, confidence, confidence, CONFIDENCE_RANGE, side, kernel_size), img_size, backend))


def wnf_slice(query_points, slice_range=(0.5, 0.6)):
    """the mask of render_wnf_points: slice_range[0] < q[:, 1] < slice_range[1] (numpy array or torch tensor, as the queries)"""
    return (slice_range[0] < query_points[..., 1]) & (query_points[..., 1] < slice_range[1])


def render_wnf_points(query_points, wnf_values, slice_range=(0.5, 0.6), side="front", img_size=256, kernel_size=4, backend="device"):
    assert side == "front"
    sel = wnf_slice(query_points, slice_range)
    return render_batch([image_spec(query_points[sel], side, kernel_size, values=wnf_values[sel], vrange=WNF_RANGE)], img_size, backend)[0]


def wnf_pair_specs(query_points, gt_wnf, pred_wnf, kernel_size=4):
    """the two images of render_wnf_points_pair: the slice of the queries coloured by the target and by the prediction"""
    sel = wnf_slice(query_points)
    q = query_points[sel]
    return scalar_pair_specs(q, q, gt_wnf[sel], pred_wnf[sel], WNF_RANGE, kernel_size=kernel_size)


def render_wnf_points_pair(query_points, gt_wnf, pred_wnf, img_size=256, backend="device"):
    return _pair(render_batch(wnf_pair_specs(query_points, gt_wnf, pred_wnf), img_size, backend))


def get_vis_idxs(batch_idx, batch_size=None, this_batch_size=None, vis_per_items=1, max_vis_per_epoch=None):
    """-> (global_idxs, selected_idxs, vis_idxs): garment i of the batch has the global index batch_size * batch_idx + i; it is drawn when that is a
    multiple of vis_per_items and its quotient, the vis_idx, is below max_vis_per_epoch"""
    assert (batch_size is not None) or (this_batch_size is not None)
    if this_batch_size is None:
        this_batch_size = batch_size
    if batch_size is None:
        batch_size = this_batch_size
    global_idxs = [batch_size * batch_idx + i for i in range(this_batch_size)]
    picked = [(i, g // vis_per_items) for i, g in enumerate(global_idxs) if g % vis_per_items == 0 and g // vis_per_items < max_vis_per_epoch]
    return global_idxs, [i for i, _ in picked], [v for _, v in picked]


# ------------------------------------------------------------------------------------------------ vis_batch
def monitor_selection(model, batch_idx, this_batch_size, is_train):
    """-> [(garment of the batch, label)]: the reference's selection, from the model's vis_per_items / max_vis_per_epoch_* / batch_size"""
    if model.vis_per_items <= 0:
        return []
    limit = model.max_vis_per_epoch_train if is_train else model.max_vis_per_epoch_val
    _, selected, vis = get_vis_idxs(batch_idx, batch_size=model.batch_size, this_batch_size=this_batch_size, vis_per_items=model.vis_per_items,
                                    max_vis_per_epoch=limit)
    return [(i, ("train_" if is_train else "val_") + str(v)) for i, v in zip(selected, vis)]


def garment_rows(batch):
    """-> rows(t, i): the rows of garment i in a per-point tensor of the batch"""
    sizes = batch.sizes
    starts = np.concatenate([[0], np.cumsum(sizes)])
    return lambda t, i: t[int(starts[i]):int(starts[i + 1])]


def grip_row(pc, pred_nocs):
    """the predicted NOCS of the point nearest the gripper (the cloud is in the gripper's frame: argmin |pos|)"""
    import torch
    return pred_nocs[torch.argmin(torch.norm(pc, p=None, dim=1))]


def nocs_monitor_specs(rows, i, batch, pred_nocs, pred_grip_nn=None, confidence=None, kernel_size=4):
    """garment i's images of the first stage's vis_batch: the NOCS pair with its grip points, then the confidence pair when there is a confidence"""
    gt, pred = rows(batch.y, i), rows(pred_nocs, i)
    specs = nocs_pair_specs(gt, pred, batch.nocs_grip_point[i], grip_row(rows(batch.pos, i), pred), None if pred_grip_nn is None else pred_grip_nn[i],
                            kernel_size=kernel_size)
    if confidence is not None:
        c = rows(confidence, i)[:, 0].contiguous()
        specs += scalar_pair_specs(gt, pred, c, c, CONFIDENCE_RANGE, kernel_size=kernel_size)
    return specs


def compose(images, per_label):
    """(I, S, S, 4) images, per_label of them per garment in pairs -> one (rows * S, 2 * S, 4) image per garment: pairs side by side, one above the next"""
    out = []
    for g in range(0, len(images), per_label):
        out.append(np.concatenate([_pair(images[j:j + 2]) for j in range(g, g + per_label, 2)], axis=0))
    return out


# ------------------------------------------------------------------------------------------------ PNG
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def to_uint8(img):
    """uint8 = trunc(clip(v, 0, 1) * 255)"""
    return (np.clip(np.asarray(img, dtype=np.float32), 0, 1) * np.float32(255)).astype(np.uint8)


def write_png(path, img):
    """an (H, W, 4) float image in [0, 1] (or uint8) as an 8-bit RGBA PNG: filter 0 on every row, the standard library's zlib"""
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError(f"write_png: expected an (H, W, 4) image, got {img.shape}")
    if img.dtype != np.uint8:
        img = to_uint8(img)
    h, w = img.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * 4)], axis=1).tobytes()

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def read_png(path):
    """-> (H, W, 4) uint8 of an 8-bit RGBA PNG whose rows all use filter 0 (what write_png writes); every chunk's CRC is verified"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f"{path}: not a PNG")
    pos, header, idat, ended = 8, None, b"", False
    while pos < len(data):
        (n,), kind = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(kind + body) & 0xFFFFFFFF != crc:
            raise ValueError(f"{path}: bad CRC in chunk {kind!r}")
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        elif kind == b"IEND":
            ended = True
        pos += 12 + n
    if header is None or not ended:
        raise ValueError(f"{path}: missing IHDR / IEND")
    w, h, depth, colour, _, _, interlace = header
    if (depth, colour, interlace) != (8, 6, 0):
        raise ValueError(f"{path}: only 8-bit RGBA without interlace is read")
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 4 * w)
    if rows[:, 0].any():
        raise ValueError(f"{path}: only filter 0 is read")
    return rows[:, 1:].reshape(h, w, 4).copy()


def epoch_writer(model, output_dir, epoch, is_train):
    """-> hook(batch_idx, batch, result) writing model.vis_batch's images of that batch under <output_dir>/vis/epoch_<NNN>/, or None when the model
    draws nothing (vis_per_items <= 0, or the subset's limit is 0): the loops then run exactly as without monitors"""
    if model.vis_per_items <= 0 or (model.max_vis_per_epoch_train if is_train else model.max_vis_per_epoch_val) <= 0:
        return None

    def hook(batch_idx, batch, result):
        write_monitor_images(output_dir, epoch, model.vis_batch(batch, batch_idx, result, is_train=is_train))
    return hook


def write_monitor_images(output_dir, epoch, images):
    """{label: image} -> <output_dir>/vis/epoch_<NNN>/<label>.png"""
    for label, img in images.items():
        write_png(os.path.join(output_dir, "vis", "epoch_%03d" % epoch, label + ".png"), img)
