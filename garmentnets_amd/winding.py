"""The generalised winding number of a triangle mesh: the quantity the WNF stage regresses (volume/nocs_winding_number_field,
volume/sim_nocs_winding_number_field of a dataset store).

Definition (normative; csrc/winding.hip follows it operation for operation).  For a query q and a face (v0, v1, v2), all fp64, with
a = v0 - q, b = v1 - q, c = v2 - q (one subtraction per component):

    la = sqrt((a.x*a.x + a.y*a.y) + a.z*a.z)                    (lb, lc alike)
    cr = (b.y*c.z - b.z*c.y,  b.z*c.x - b.x*c.z,  b.x*c.y - b.y*c.x)
    num = (a.x*cr.x + a.y*cr.y) + a.z*cr.z
    dab = (a.x*b.x + a.y*b.y) + a.z*b.z                          (dbc, dca alike)
    den = (((la*lb)*lc + dab*lc) + dbc*la) + dca*lb
    omega = 2 * atan2(num, den)                                  (Van Oosterom-Strackee)
    w(q) = (0 + omega_0 + omega_1 + ... in face-index order) / (4 pi)

Every operation is rounded on its own (numpy never contracts to fma; the kernel uses _rn intrinsics), so `num` and `den` are the same bits
here and on the device and only atan2 may differ between the two.  IEEE atan2 is the edge rule: a query on a mesh vertex gets
atan2(+-0, +0) = +-0 from the incident faces (the first term of den is +0 there); a query inside a face's plane sits on the
discontinuity of the function itself.  An empty mesh gives 0.

Lattice node (i, j, k) of a (D, H, W) volume is the point (i/(D-1), j/(H-1), k/(W-1)), divided in fp64: the convention
io.dataset.nocs_grid_sample reads a volume with.
"""
import numpy as np

FOUR_PI = 4.0 * np.pi
_CHUNK_PAIRS = 1 << 21            # (queries x faces) entries per block of the reference: ~16 MiB per temporary


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _mesh_arrays(verts, faces):
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces)
    if verts.ndim != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts: expected an (N, 3) array, got {verts.shape}")
    if faces.size == 0:
        faces = np.zeros((0, 3), dtype=np.int64)
    if faces.dtype.kind not in "iu":
        raise TypeError(f"faces: expected an integer array, got {faces.dtype}")
    if faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces: expected an (F, 3) array, got {faces.shape}")
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise IndexError("winding number: a face index is out of bounds for its mesh's vertices")
    return verts, faces


def winding_number_reference(queries, verts, faces):
    """w(q) of the definition above for every row of `queries` (M, 3) -> (M,) float64.  numpy, fp64, the faces summed sequentially in index
    order (np.cumsum adds one element after the other)."""
    return solid_angle_sum_reference(queries, verts, faces) / FOUR_PI


def solid_angle_sum_reference(queries, verts, faces):
    """0 + omega_0 + omega_1 + ... in face-index order for every row of `queries` (M, 3) -> (M,) float64: winding_number_reference before its division
    by 4 pi (targets.query_targets_reference adds these per chunk of faces)"""
    queries = np.asarray(queries, dtype=np.float64)
    if queries.ndim != 2 or queries.shape[1] != 3:
        raise ValueError(f"queries: expected an (M, 3) array, got {queries.shape}")
    verts, faces = _mesh_arrays(verts, faces)
    out = np.zeros(len(queries), dtype=np.float64)
    if len(faces) == 0 or len(queries) == 0:
        return out
    tri = [[verts[faces[:, k], c][None, :] for c in range(3)] for k in range(3)]          # tri[k][c]: (1, F)
    step = max(1, _CHUNK_PAIRS // len(faces))
    for s in range(0, len(queries), step):
        q = [queries[s:s + step, c][:, None] for c in range(3)]                          # (m, 1)
        a, b, c = ([tri[k][x] - q[x] for x in range(3)] for k in range(3))
        la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
        cr = (b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0])
        num = _dot(a, cr)
        dab, dbc, dca = _dot(a, b), _dot(b, c), _dot(c, a)
        den = (((la * lb) * lc + dab * lc) + dbc * la) + dca * lb
        omega = 2.0 * np.arctan2(num, den)
        out[s:s + step] = 0.0 + np.cumsum(omega, axis=1)[:, -1]
    return out


def lattice_points(shape):
    """the (D*H*W, 3) float64 points of a (D, H, W) lattice over the unit cube, in C order of the volume"""
    D, H, W = (int(n) for n in shape)
    if min(D, H, W) < 2:
        raise ValueError(f"lattice {(D, H, W)}: every axis needs at least 2 nodes")
    ax = [np.arange(n, dtype=np.float64) / np.float64(n - 1) for n in (D, H, W)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


def winding_field_reference(verts, faces, shape):
    """the winding number of (verts, faces) at every node of a `shape` = (D, H, W) lattice -> (D, H, W) float32 (float64 values rounded once)"""
    return winding_number_reference(lattice_points(shape), verts, faces).reshape(tuple(int(n) for n in shape)).astype(np.float32)


def winding_field(meshes, shape, backend=None):
    """the fields of a list of meshes [(verts, faces)] (numpy arrays) -> (B, D, H, W) float32 numpy array.  backend None / "hip": all meshes
    in one launch of gn_winding_field_batch on the current device; "numpy": winding_field_reference per mesh.  The two differ by what atan2
    differs ("Winding numbers")."""
    shape = tuple(int(n) for n in shape)
    if backend in (None, "hip"):
        from . import ops
        on_dev = ops.meshes_f64(meshes)
        if not on_dev:
            return np.zeros((0,) + shape, dtype=np.float32)
        return ops.winding_field_batch(on_dev, shape).cpu().numpy()
    if backend != "numpy":
        raise ValueError(f"backend {backend!r}: expected 'hip' or 'numpy'")
    return np.stack([winding_field_reference(v, f, shape) for v, f in meshes]) if len(meshes) else np.zeros((0,) + shape, dtype=np.float32)
