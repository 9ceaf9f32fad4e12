"""Point clouds from meshes: the multi-view partial depth clouds a dataset store holds as point_cloud/{point, nocs, rgb, sizes}, rendered from the
garment mesh (DESIGN.md "Point clouds from meshes").  The reference ships these clouds and no code that made them, so the definitions are this
package's own: a ring of pinhole cameras around the store's bounding box, the mesh images' integer coverage behind each of them, perspective-correct
depth and labels, and the covered pixels of every view, in raster order, as the cloud.

  camera_ring(aabb, ...)                         the cameras: host trigonometry, once; the device reads their fp64 records
  render_point_clouds(meshes, cameras, S, ...)   every garment of a call times every view in one launch set (ops.depth_render_batch, ops.depth_cloud),
                                                 or, backend="numpy", the restatement below: the same operations in the same order, bit for bit

The restatement spells every sum whose order the definition fixes; it uses neither `@` nor einsum there (a BLAS may fuse or reorder).  The coverage
rules, the drawn faces, the index image and the winner's weights live in raster.py, shared with visualize.py; this module brings its pinhole, the
near plane, the inverse depth, the mixes and the headlight.
"""
import math

import numpy as np

from . import raster
from .raster import _host
from .visualize import DEFAULT_AMBIENT

DEFAULT_FOV, DEFAULT_ELEVATION = 45.0, 20.0     # degrees; a look, not a measurement: how much of a view the garment fills, and from how high it is seen
DEFAULT_BASE_COLOR = (0.5, 0.5, 0.5)            # a look as well: the grey the headlight shades
CLOUD_ARRAYS = ("point", "nocs", "rgb", "sizes")


# ------------------------------------------------------------------------------------------------ cameras
def camera_ring(aabb, num_views=4, img_size=256, fov=DEFAULT_FOV, elevation=DEFAULT_ELEVATION, azimuth0=0.0, distance=None):
    """`num_views` cameras on a ring around the box aabb ((2, 3): its corners), looking at its centre with up = +z: azimuth azimuth0 + 360 k / V
    degrees about the z axis, `elevation` degrees above the xy plane, a square image of `img_size` pixels over `fov` degrees.  The default distance is
    derived: d = r / sin(fov / 2), r the box's half-diagonal, so the box's bounding sphere fits the view cone (which the square image contains);
    near = (d - r) / 2, f = (S / 2) / tan(fov / 2), c = S / 2.
    -> [{"R": (3, 3) fp64 world -> camera (x right, y down, z forward), "t": (3,), "f", "c", "near"}]"""
    box = np.asarray(aabb, dtype=np.float64).reshape(2, 3)
    S, V = int(img_size), int(num_views)
    if V < 1 or S < 1:
        raise ValueError(f"camera_ring: num_views={V} and img_size={S} must be positive")
    if not (0.0 < fov < 180.0) or not (-90.0 < elevation < 90.0):
        raise ValueError(f"camera_ring: fov={fov} outside (0, 180) or elevation={elevation} outside (-90, 90): the up vector is +z")
    target, r = (box[0] + box[1]) / 2, float(np.linalg.norm(box[1] - box[0])) / 2
    half = math.radians(fov) / 2
    d = r / math.sin(half) if distance is None else float(distance)
    if not (d > r and math.isfinite(d)):
        raise ValueError(f"camera_ring: distance {d} does not clear the bounding sphere (radius {r}): near = (d - r) / 2 must be positive")
    f, el = (S / 2) / math.tan(half), math.radians(elevation)
    cams = []
    for k in range(V):
        az = math.radians(azimuth0 + 360.0 * k / V)
        out = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        forward = -out
        right = np.cross(forward, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(forward, right)
        R = np.stack([right, down / np.linalg.norm(down), forward])
        cams.append({"R": R, "t": -(R @ (target + d * out)), "f": float(f), "c": S / 2, "near": (d - r) / 2})
    return cams


def camera_attrs(cameras):
    """the records as JSON-able values (a store's point_cloud attributes)"""
    return [{"R": np.asarray(c["R"], np.float64).reshape(3, 3).tolist(), "t": np.asarray(c["t"], np.float64).reshape(3).tolist(), "f": float(c["f"]),
             "c": float(c["c"]), "near": float(c["near"])} for c in cameras]


# ------------------------------------------------------------------------------------------------ the numpy restatement
def to_camera(points, cam):
    """(N, 3) fp32 -> (N, 3) fp64: cam[j] = ((R[j][0] x + R[j][1] y) + R[j][2] z) + t[j], every operation rounded on its own"""
    p = _host(points).reshape(-1, 3).astype(np.float64)
    R, t = np.asarray(cam["R"], dtype=np.float64).reshape(3, 3), np.asarray(cam["t"], dtype=np.float64).reshape(3)
    return np.stack([((R[j, 0] * p[:, 0] + R[j, 1] * p[:, 1]) + R[j, 2] * p[:, 2]) + t[j] for j in range(3)], axis=1)


def _depth_faces(verts, faces, cam):
    """raster.drawn_faces behind the pinhole: screen = (f * x) / z + c, a vertex nearer than the near plane is not seen"""
    fl, c, near = np.float64(cam["f"]), np.float64(cam["c"]), np.float64(cam["near"])

    def project(v):
        pc = to_camera(v, cam)
        return pc, (fl * pc[:, 0]) / pc[:, 2] + c, (fl * pc[:, 1]) / pc[:, 2] + c, pc[:, 2] >= near
    return raster.drawn_faces(verts, faces, project)


def _inverse_depth(wa, wb, wc, z):
    """(q_a, q_b, q_c, q) of the covered samples: i_k = 1 / z_k, q_k = double(w_k) * i_k, q = (q_a + q_b) + q_c.  z: (P, 3)"""
    qa, qb, qc = (w.astype(np.float64) * (1.0 / z[:, k]) for k, w in enumerate((wa, wb, wc)))
    return qa, qb, qc, (qa + qb) + qc


def render_depth_idx_numpy(verts, faces, cam, S):
    """-> the index image (S, S) uint32: per pixel the covering face with the largest inv = q / double(area2), the lowest index among equal ones"""
    index, _, fx, fy, pc = _depth_faces(verts, faces, cam)
    return raster.raster_idx(index, fx, fy, S, lambda face, wa, wb, wc: _inverse_depth(wa, wb, wc, pc[face][:, :, 2])[3] /
                             (wa + wb + wc).astype(np.float64), largest=True)[0]


def _mix(ba, bb, bc, corners):
    """((b_a A + b_b B) + b_c C) per coordinate in fp64 on the fp32 corners (P, 3 corners, 3), rounded once to fp32"""
    c = corners.astype(np.float64)
    return ((ba[:, None] * c[:, 0] + bb[:, None] * c[:, 1]) + bc[:, None] * c[:, 2]).astype(np.float32)


def depth_cloud_numpy(idx_img, verts, nocs, faces, cam, ambient=DEFAULT_AMBIENT, base_color=DEFAULT_BASE_COLOR, screen_linear=False):
    """the covered pixels of one index image in raster order -> (point (P, 3) fp32, nocs (P, 3) fp32, rgb (P, 3) uint8).  screen_linear: mix with the
    screen-space weights w_k / area2 instead of the perspective-correct ones -- NOT the definition; the tests show what it breaks"""
    index, f, fx, fy, pc = _depth_faces(verts, faces, cam)
    Y, _, row, wa, wb, wc = raster.winner_weights(idx_img, index, fx, fy)
    if len(Y) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8)
    qa, qb, qc, q = _inverse_depth(wa, wb, wc, pc[row][:, :, 2])
    if screen_linear:
        qa, qb, qc, q = wa.astype(np.float64), wb.astype(np.float64), wc.astype(np.float64), (wa + wb + wc).astype(np.float64)
    ba, bb, bc = qa / q, qb / q, qc / q
    point = _mix(ba, bb, bc, _host(verts).reshape(-1, 3)[f[row]])
    label = _mix(ba, bb, bc, _host(nocs).reshape(-1, 3)[f[row]])
    nx, ny, nz = raster.face_normals(pc[row])
    amb = np.float64(np.float32(ambient))
    with np.errstate(all="ignore"):
        p = to_camera(point, cam)
        nn = (nx * nx + ny * ny) + nz * nz
        pp = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
        dot = (nx * p[:, 0] + ny * p[:, 1]) + nz * p[:, 2]
        root = np.sqrt(nn * pp)
        lit = np.isfinite(point).all(axis=1) & (root > 0) & np.isfinite(root)
        shade = np.where(lit, amb + (1.0 - amb) * (np.abs(dot) / root), amb)
        sh = np.float32(255) * shade.astype(np.float32)
        r = np.rint(sh[:, None] * np.asarray(base_color, dtype=np.float32).reshape(1, 3))
        rgb = np.where(r >= 255, np.float32(255), np.where(r > 0, r, np.float32(0))).astype(np.uint8)         # NaN -> 0
    return point, label, rgb


# ------------------------------------------------------------------------------------------------ the public entry
def _split(arrays, sizes, n_views):
    """the concatenated rows of G * n_views images -> one {"point", "nocs", "rgb", "sizes"} per garment"""
    point, label, rgb = arrays
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, n_views)
    ends = np.cumsum(sizes.sum(axis=1))
    return [{"point": point[e - s.sum():e], "nocs": label[e - s.sum():e], "rgb": rgb[e - s.sum():e], "sizes": s.copy()} for e, s in zip(ends, sizes)]


def render_point_clouds(meshes, cameras, img_size=256, base_color=DEFAULT_BASE_COLOR, ambient=DEFAULT_AMBIENT, backend="device", device=None):
    """meshes: [(verts (V, 3) fp32, nocs_verts (V, 3) fp32, faces (F, 3) int32)], numpy arrays or torch tensors; cameras: camera_ring's records, the
    same for every garment.  -> per garment {"point" (N, 3) fp32, "nocs" (N, 3) fp32, "rgb" (N, 3) uint8, "sizes" (views,) int64} on the host: the views
    back to back in the cameras' order, within a view the covered pixels in raster order.  backend "device": every garment times every view in ONE
    launch set (the rasteriser, the row counts and their scan, the write pass); "numpy": the restatement"""
    meshes, cameras, S = list(meshes), list(cameras), int(img_size)
    if backend not in ("device", "numpy"):
        raise ValueError(f"backend={backend!r}: expected 'device' or 'numpy'")
    if len(base_color) != 3:
        raise ValueError("base_color: expected 3 floats (RGB)")
    for i, (v, n, _) in enumerate(meshes):
        if tuple(np.shape(v)) != tuple(np.shape(n)):
            raise ValueError(f"render_point_clouds: mesh {i}: one NOCS row per vertex ({tuple(np.shape(v))} verts, {tuple(np.shape(n))} nocs)")
    nv = len(cameras)
    if not meshes or not nv:
        return [{"point": np.zeros((0, 3), np.float32), "nocs": np.zeros((0, 3), np.float32), "rgb": np.zeros((0, 3), np.uint8),
                 "sizes": np.zeros(nv, np.int64)} for _ in meshes]
    if backend == "numpy":
        rows, sizes = [], []
        for v, n, f in meshes:
            for cam in cameras:
                rows.append(depth_cloud_numpy(render_depth_idx_numpy(v, f, cam, S), v, n, f, cam, ambient, base_color))
                sizes.append(len(rows[-1][0]))
        return _split([np.concatenate([r[k] for r in rows]) for k in range(3)], sizes, nv)
    from . import ops

    verts, faces, nocs, vseg, fseg = ops.pack_meshes([(v, f, n) for v, n, f in meshes], (3,), device)
    mesh_of = np.repeat(np.arange(len(meshes), dtype=np.int32), nv)
    cams = cameras * len(meshes)
    idx = ops.depth_render_batch(verts, faces, vseg, fseg, mesh_of, cams, S)
    point, label, rgb, sizes = ops.depth_cloud(idx, verts, nocs, faces, vseg, fseg, mesh_of, cams, [float(ambient)] * len(cams),
                                               [tuple(float(c) for c in base_color)] * len(cams))
    return _split([point.cpu().numpy(), label.cpu().numpy(), rgb.cpu().numpy()], sizes, nv)
