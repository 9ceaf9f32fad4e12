"""The mesh rasteriser's numpy restatement, once (DESIGN.md "Mesh images", "Point clouds from meshes"): the integer coverage rules, the drawn faces
behind a projection, the index image under a per-sample value, the winner's weights from an index image, and the camera-space face normals.  The
callers bring what differs: visualize.py its axis cameras, depth, colour mix and shade; point_cloud.py its pinhole, near plane, inverse depth and
headlight.  Numpy only: neither torch nor the library is needed.  Every sum whose order the definitions fix is parenthesised; no `@`, no einsum.
"""
import numpy as np

DEFAULT_IDX = np.uint32(0xFFFFFFFF)
MESH_SUBPIXEL = 256
MESH_COORD_LIMIT = 2 ** 24


def _host(a, dtype=np.float32):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


def _edge(px, py, qx, qy, rx, ry):
    """E(p, q, r) = (qx - px)(ry - py) - (qy - py)(rx - px) in int64"""
    return (qx - px) * (ry - py) - (qy - py) * (rx - px)


def _owns(px, py, qx, qy):
    """the directed edge p -> q owns the samples on it: dy > 0 or (dy == 0 and dx < 0)"""
    dx, dy = qx - px, qy - py
    return (dy > 0) | ((dy == 0) & (dx < 0))


def _mesh_weights(fx, fy, px, py):
    """-> (w_a, w_b, w_c, covered) of the samples (px, py) in the faces (fx, fy) [.., 3], all int64"""
    ax, ay, bx, by, cx, cy = fx[..., 0], fy[..., 0], fx[..., 1], fy[..., 1], fx[..., 2], fy[..., 2]
    wa, wb, wc = _edge(bx, by, cx, cy, px, py), _edge(cx, cy, ax, ay, px, py), _edge(ax, ay, bx, by, px, py)
    covered = ((wa > 0) | ((wa == 0) & _owns(bx, by, cx, cy))) & ((wb > 0) | ((wb == 0) & _owns(cx, cy, ax, ay))) & \
        ((wc > 0) | ((wc == 0) & _owns(ax, ay, bx, by)))
    return wa, wb, wc, covered


def _samples(X, Y):
    """the pixels' sample points in subpixel units: 256 X + 128"""
    return MESH_SUBPIXEL * X + MESH_SUBPIXEL // 2, MESH_SUBPIXEL * Y + MESH_SUBPIXEL // 2


def drawn_faces(verts, faces, project):
    """the drawn faces in positive orientation -> (index [D] int64, vertex indices [D, 3] after the swap, fx, fy [D, 3] int64, cam [D, 3, 3] fp64).
    project(v (N, 3) fp32) -> (cam (N, 3) fp64, screen x, y (N,) fp64 in pixels, seen (N,) bool).  Not drawn: a face with a vertex index out of range,
    a non-finite or unseen vertex, a fixed-point coordinate beyond 2^24 in magnitude, or zero area"""
    v = _host(verts).reshape(-1, 3)
    f = _host(faces, np.int64).reshape(-1, 3)
    keep = np.flatnonzero(((f >= 0) & (f < len(v))).all(axis=1))
    f = f[keep]
    with np.errstate(all="ignore"):
        cam, sx, sy, seen = project(v)
        ok = (np.isfinite(v).all(axis=1) & seen)[f].all(axis=1)
        fx = np.rint(sx * np.float64(MESH_SUBPIXEL))[f]                                 # half to even
        fy = np.rint(sy * np.float64(MESH_SUBPIXEL))[f]
        ok &= (np.abs(fx) <= MESH_COORD_LIMIT).all(axis=1) & (np.abs(fy) <= MESH_COORD_LIMIT).all(axis=1)
    keep, f, cam = keep[ok], f[ok], cam[f[ok]]                                          # cam: (D, 3 corners, 3 coordinates)
    fx, fy = fx[ok].astype(np.int64), fy[ok].astype(np.int64)
    area2 = _edge(fx[:, 0], fy[:, 0], fx[:, 1], fy[:, 1], fx[:, 2], fy[:, 2])
    drawn = area2 != 0
    keep, f, cam, fx, fy, area2 = keep[drawn], f[drawn], cam[drawn], fx[drawn], fy[drawn], area2[drawn]
    order = np.where((area2 < 0)[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))    # two-sided: b and c swap, with everything they carry
    rows = np.arange(len(keep))[:, None]
    return keep, f[rows, order], fx[rows, order], fy[rows, order], cam[rows, order]


def raster_idx(index, fx, fy, S, value, largest):
    """-> (index image (S, S) uint32, the winners' values (S, S) fp64): per pixel the face covering its sample with the largest (or the smallest)
    value(face row (P,), w_a, w_b, w_c (P,) int64) -> (P,) fp64, the lowest index among equal ones; 0xFFFFFFFF and -inf (+inf) where nobody covers"""
    img = np.full((S, S), DEFAULT_IDX, dtype=np.uint32)
    vimg = np.full((S, S), -np.inf if largest else np.inf)
    half = MESH_SUBPIXEL // 2                                                           # the pixels whose samples lie in the face's box, within the image
    xlo = np.maximum(-((-(fx.min(axis=1) - half)) // MESH_SUBPIXEL), 0)
    xhi = np.minimum((fx.max(axis=1) - half) // MESH_SUBPIXEL, S - 1)
    ylo = np.maximum(-((-(fy.min(axis=1) - half)) // MESH_SUBPIXEL), 0)
    yhi = np.minimum((fy.max(axis=1) - half) // MESH_SUBPIXEL, S - 1)
    wd, ht = np.maximum(xhi - xlo + 1, 0), np.maximum(yhi - ylo + 1, 0)
    n = wd * ht
    if n.sum() == 0:
        return img, vimg
    face = np.repeat(np.arange(len(index)), n)                                          # every (face, pixel of its box) pair
    local = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    X, Y = xlo[face] + local % wd[face], ylo[face] + local // wd[face]
    wa, wb, wc, covered = _mesh_weights(fx[face], fy[face], *_samples(X, Y))
    face, X, Y, wa, wb, wc = face[covered], X[covered], Y[covered], wa[covered], wb[covered], wc[covered]
    val = value(face, wa, wb, wc)
    pixel = Y * S + X
    order = np.lexsort((index[face], -val if largest else val, pixel))                  # per pixel: the winning value, then the lowest index
    first = np.ones(order.size, dtype=bool)
    first[1:] = pixel[order][1:] != pixel[order][:-1]
    img.reshape(-1)[pixel[order][first]] = index[face][order][first].astype(np.uint32)
    vimg.reshape(-1)[pixel[order][first]] = val[order][first]
    return img, vimg


def winner_weights(idx_img, index, fx, fy):
    """the covered pixels of an index image in raster order (Y, then X) -> (Y, X, row of the winner among the drawn faces, w_a, w_b, w_c int64): the
    winner is a drawn face that covers the pixel's sample, so its weights are recomputed, not stored"""
    Y, X = np.nonzero(idx_img != DEFAULT_IDX)
    row = np.searchsorted(index, idx_img[Y, X].astype(np.int64))
    wa, wb, wc, covered = _mesh_weights(fx[row], fy[row], *_samples(X, Y))
    assert covered.all() and np.array_equal(index[row], idx_img[Y, X])
    return Y, X, row, wa, wb, wc


def face_normals(cam):
    """(P, 3 corners, 3) fp64 -> (n_x, n_y, n_z) of n = (B - A) x (C - A)"""
    u, w = cam[:, 1] - cam[:, 0], cam[:, 2] - cam[:, 0]
    return u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
