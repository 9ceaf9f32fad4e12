"""The distance from a lattice node to a triangle mesh, and the three training targets made of it: volume/nocs_distance_field,
volume/nocs_signed_distance_field and volume/nocs_occupancy_grid of a dataset store ("Distance, signed-distance and occupancy targets").

Definition of d2 (normative; csrc/eval_dist.hip pm_stage_tile / pm_sqdist follow it operation for operation).  All fp64, every operation
rounded on its own, a three-term dot product summed as (x*x' + y*y') + z*z'.  Per face (v0, v1, v2), once:

    e0 = v1 - v0,  e1 = v2 - v0,  e2 = v2 - v1
    a = e0.e0,  b = e0.e1,  c = e1.e1,  l2 = e2.e2,  det = a*c - b*b
    ia, ic, ie2, idet = 1/a, 1/c, 1/l2, 1/det          (0 where the value is not > 0)

Per (query q, face):

    w = q - v0,  d0 = w.e0,  d1 = w.e1,  u = q - v1
    seg(w, e, wd, inv):  t = fmin(fmax(wd*inv, 0), 1);  r = w - t*e;  r.r          (the clamped distance to an edge)
    s0 = seg(w, e0, d0, ia),  s1 = seg(w, e1, d1, ic),  s2 = seg(u, e2, u.e2, ie2)
    s = (c*d0 - b*d1)*idet,  t = (a*d1 - b*d0)*idet
    r = (w - s*e0) - t*e1,  plane = r.r
    inside = idet > 0 and s >= 0 and t >= 0 and s + t <= 1
    d = fmin(plane, fmin(fmin(s0, s1), s2)) if inside else fmin(fmin(s0, s1), s2)

d2(q) is the strict `<` minimum of d over the faces in index order, so ties go to the lowest face index; an empty mesh gives (+inf, -1); a NaN
query gives (NaN, -1).  Degenerate faces are measured as their edges.

The targets, from d2 and the stored float32 winding field w32 of the same sample and size (THIS PACKAGE'S OWN rules: the reference ships the
volumes, not how they were made):

    nocs_distance_field          float32(sqrt(d2))                                    the root in fp64, rounded once
    nocs_signed_distance_field   float32(clip(1 - 2*float64(w32), -1, 1) * sqrt(d2))  minus the distance inside a closed mesh, plus outside
    nocs_occupancy_grid          float32(w32 > 0.5)

The sign factor is 1 - 2 w wherever w lies in [0, 1].  The winding number of an OPEN mesh leaves that interval (outside, away from the opening, it
is minus the solid angle of the missing patch over 4 pi; between overlapping sheets it passes 1), and the unclipped factor would then give a
magnitude LARGER than the distance to the mesh; clipped, |signed| <= distance holds at every node, exactly (a factor of magnitude <= 1 and two
monotone roundings), and nothing else changes: the field is still continuous, zero on the garment and where w crosses 0.5.

The lattice is winding.lattice_points: node (i, j, k) of a (D, H, W) volume is (i/(D-1), j/(H-1), k/(W-1)), divided in fp64.
"""
import numpy as np

from .winding import _CHUNK_PAIRS, _dot, _mesh_arrays, lattice_points

DISTANCE_GROUP = "nocs_distance_field"
SIGNED_DISTANCE_GROUP = "nocs_signed_distance_field"
OCCUPANCY_GROUP = "nocs_occupancy_grid"
OCCUPANCY_LEVEL = 0.5                   # of the winding field: the level --marching_cubes meshes


def _rcp_or_zero(x):
    return np.where(x > 0.0, 1.0 / np.where(x > 0.0, x, 1.0), 0.0)


def _seg(w, e, wd, inv):
    t = np.fmin(np.fmax(wd * inv, 0.0), 1.0)
    r = [w[x] - t * e[x] for x in range(3)]
    return _dot(r, r)


def point_mesh_sqdist_reference(queries, verts, faces):
    """(face_idx int32 (M,), d2 float64 (M,)) of the definition above for every row of `queries` (M, 3).  numpy, fp64, in blocks of queries;
    np.argmin returns the first minimum: the lowest face index."""
    queries = np.asarray(queries, dtype=np.float64)
    if queries.ndim != 2 or queries.shape[1] != 3:
        raise ValueError(f"queries: expected an (M, 3) array, got {queries.shape}")
    verts, faces = _mesh_arrays(verts, faces)
    idx = np.full(len(queries), -1, dtype=np.int32)
    d2 = np.full(len(queries), np.inf, dtype=np.float64)
    if len(faces) == 0 or len(queries) == 0:
        d2[np.isnan(queries).any(axis=1)] = np.nan
        return idx, d2
    p = [[verts[faces[:, k], x][None, :] for x in range(3)] for k in range(3)]             # p[k][x]: (1, F)
    e0, e1, e2 = ([p[i][x] - p[j][x] for x in range(3)] for i, j in ((1, 0), (2, 0), (2, 1)))
    a, b, c, l2 = _dot(e0, e0), _dot(e0, e1), _dot(e1, e1), _dot(e2, e2)
    with np.errstate(all="ignore"):
        idet, ia, ic, ie2 = _rcp_or_zero(a * c - b * b), _rcp_or_zero(a), _rcp_or_zero(c), _rcp_or_zero(l2)
    step = max(1, _CHUNK_PAIRS // len(faces))
    for s0_ in range(0, len(queries), step):
        q = [queries[s0_:s0_ + step, x][:, None] for x in range(3)]                      # (m, 1)
        with np.errstate(all="ignore"):
            w = [q[x] - p[0][x] for x in range(3)]
            d0, d1 = _dot(w, e0), _dot(w, e1)
            s0, s1 = _seg(w, e0, d0, ia), _seg(w, e1, d1, ic)
            u = [q[x] - p[1][x] for x in range(3)]
            s2 = _seg(u, e2, _dot(u, e2), ie2)
            s, t = (c * d0 - b * d1) * idet, (a * d1 - b * d0) * idet
            r = [(w[x] - s * e0[x]) - t * e1[x] for x in range(3)]
            plane = _dot(r, r)
            inside = (idet > 0.0) & (s >= 0.0) & (t >= 0.0) & (s + t <= 1.0)
            seg = np.fmin(np.fmin(s0, s1), s2)
            d = np.where(inside, np.fmin(plane, seg), seg)
        d = np.where(np.isnan(d), np.inf, d)                                             # `d < best` is false for a NaN: never taken
        best = np.argmin(d, axis=1)
        val = d[np.arange(len(best)), best]
        idx[s0_:s0_ + step] = np.where(val < np.inf, best, -1)
        d2[s0_:s0_ + step] = val
    d2[np.isnan(queries).any(axis=1)] = np.nan
    return idx, d2


def distance_field_reference(verts, faces, shape):
    """(d2 float64 (D, H, W), face_idx int32 (D, H, W)) of the mesh (verts, faces) at every node of a `shape` = (D, H, W) lattice"""
    shape = tuple(int(n) for n in shape)
    idx, d2 = point_mesh_sqdist_reference(lattice_points(shape), verts, faces)
    return d2.reshape(shape), idx.reshape(shape)


# ------------------------------------------------------------------------------------------------ the three targets (both backends call these)
def distance_volume(d2):
    """nocs_distance_field: float32(sqrt(d2))"""
    return np.sqrt(np.asarray(d2, dtype=np.float64)).astype(np.float32)


def signed_distance_volume(d2, w32):
    """nocs_signed_distance_field: float32(clip(1 - 2 w32, -1, 1) sqrt(d2)), in fp64 and rounded once.  Zero on the mesh and where the winding field
    crosses 0.5; never larger in magnitude than distance_volume(d2)."""
    w32 = np.asarray(w32)
    if w32.dtype != np.float32:
        raise TypeError(f"the winding field is the stored float32 volume, got {w32.dtype}")
    sign = np.clip(1.0 - 2.0 * w32.astype(np.float64), -1.0, 1.0)
    return (sign * np.sqrt(np.asarray(d2, dtype=np.float64))).astype(np.float32)


def occupancy_volume(w32):
    """nocs_occupancy_grid: float32(w32 > 0.5)"""
    w32 = np.asarray(w32)
    if w32.dtype != np.float32:
        raise TypeError(f"the winding field is the stored float32 volume, got {w32.dtype}")
    return (w32 > np.float32(OCCUPANCY_LEVEL)).astype(np.float32)


def derived_volume(group, d2, w32):
    """the float32 volume of one of the three groups; d2 / w32 may be None where the group does not read it"""
    if group == DISTANCE_GROUP:
        return distance_volume(d2)
    if group == SIGNED_DISTANCE_GROUP:
        return signed_distance_volume(d2, w32)
    if group == OCCUPANCY_GROUP:
        return occupancy_volume(w32)
    raise ValueError(f"unknown derived group {group!r}")


def distance_field(meshes, shape, backend=None):
    """the squared distances of a list of meshes [(verts, faces)] (numpy arrays) -> (d2 (B, D, H, W) float64, face_idx (B, D, H, W) int32), numpy.
    backend None / "hip": all meshes in one launch of gn_distance_field_batch on the current device; "numpy": distance_field_reference per
    mesh.  The two agree bit for bit."""
    shape = tuple(int(n) for n in shape)
    if backend not in (None, "hip", "numpy"):
        raise ValueError(f"backend {backend!r}: expected 'hip' or 'numpy'")
    if not len(meshes):
        return np.zeros((0,) + shape, dtype=np.float64), np.zeros((0,) + shape, dtype=np.int32)
    if backend == "numpy":
        fields = [distance_field_reference(v, f, shape) for v, f in meshes]
        return np.stack([d for d, _ in fields]), np.stack([i for _, i in fields])
    from . import ops
    d2, face_idx = ops.distance_field_batch(ops.meshes_f64(meshes), shape)
    return d2.cpu().numpy(), face_idx.cpu().numpy()
