"""Meshes, parameters and store builders shared by tests/test_cloth_host.py and tests/test_gpu_cloth.py (garmentnets_amd/cloth.py).  Every test passes
its parameters explicitly: none depends on a default of cloth.py."""
import numpy as np

from garmentnets_amd import cloth
from garmentnets_amd.io import zarr_store

# soft enough that a few hundred substeps move every vertex by many rest lengths, stiff enough to stay finite
PARAMS = cloth.ClothParams(gravity=9.81, h=1.0 / 300.0, damping=1.5, alpha_stretch=1e-7, alpha_bend=0.02, density=0.3)
EPS = 2.0 ** -52


def sheet(n, m, seed=0, size=0.4, jitter=0.15, flat=False):
    """an n x m vertex sheet, 2 (n - 1)(m - 1) faces, jittered by `jitter` of a cell (flat: z = 0 exactly, the sheet horizontal) -> (X (n m, 3), faces)"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(m, dtype=np.float64), indexing="ij")
    cell = size / max(n - 1, m - 1)
    X = np.stack([u * cell, v * cell, np.zeros_like(u)], axis=-1).reshape(-1, 3)
    X += rng.uniform(-jitter * cell, jitter * cell, X.shape)
    X[:, 2] = 0.0 if flat else 0.1 * size * np.sin(3.0 * X[:, 0] / size) * np.cos(2.0 * X[:, 1] / size)
    idx = np.arange(n * m).reshape(n, m)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], axis=1).reshape(-1, 3).astype(np.int32)
    return X, faces


def sheet_counts(n, m):
    """(stretch, bend) of an n x m vertex sheet: n (m - 1) + (n - 1) m grid edges and (n - 1)(m - 1) diagonals; every edge but the 2 (n - 1) + 2 (m - 1)
    on the boundary lies between two faces"""
    stretch = n * (m - 1) + (n - 1) * m + (n - 1) * (m - 1)
    return stretch, stretch - 2 * (n - 1) - 2 * (m - 1)


TRIANGLE = (np.array([[0.0, 0.0, 0.0], [0.2, 0.01, 0.03], [0.05, 0.25, -0.02]]), np.array([[0, 1, 2]], dtype=np.int32))
TWO_TRIANGLES = (np.array([[0.0, 0.0, 0.0], [0.2, 0.01, 0.03], [0.05, 0.25, -0.02], [0.27, 0.22, 0.05]]),
                 np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32))
FAN = (np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.3], [0.2, 0.0, 0.1], [-0.1, 0.2, 0.1], [-0.1, -0.2, 0.2]]),
       np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], dtype=np.int32))


def with_massless(n=5, m=4, seed=1):
    """a sheet plus two vertices that no face names (one in the middle of the array, one at its end)"""
    X, faces = sheet(n, m, seed)
    k = 7
    X = np.concatenate([X[:k], [[0.11, -0.2, 0.3]], X[k:], [[-0.3, 0.1, 0.2]]])
    return X, np.where(faces >= k, faces + 1, faces).astype(np.int32), (k, len(X) - 1)


def with_coincident(n=5, m=4, seed=2):
    """a sheet with vertex 7 moved onto vertex 6: the edge between them has len == 0 = l0 and the two faces at it have no area"""
    X, faces = sheet(n, m, seed)
    X[7] = X[6]
    return X, faces


def garment(mesh, grip=0, params=PARAMS, **kw):
    return cloth.garment(mesh[0], mesh[1], grip, params, **kw)


def python_first_fit(pairs):
    """the colouring rule of the definition, written plainly: the smallest colour no earlier constraint at either vertex has"""
    at = {}
    out = []
    for i, j in pairs:
        taken = at.setdefault(i, set()) | at.setdefault(j, set())
        c = 0
        while c in taken:
            c += 1
        out.append(c)
        at[i].add(c)
        at[j].add(c)
    return out


def write_canonical_store(path, meshes, grips=True, canonical_aabb=True):
    """a dataset store that holds canonical meshes and nothing made from them: mesh/cloth_nocs_verts, mesh/cloth_faces_tri, the attributes (grips: with
    grip_vertex_idx) and, with canonical_aabb, summary/cloth_canonical_aabb_union.  NO cloth_verts, NO cloth_aabb_union.  meshes: [(nocs, faces)]"""
    root = zarr_store.open_group(str(path))
    if canonical_aabb:
        root.require_group("summary").array("cloth_canonical_aabb_union", np.array([[-0.45, -0.2, -0.5], [0.45, 0.3, 0.4]], dtype=np.float32))
    keys = []
    for i, (nocs, faces) in enumerate(meshes):
        key = f"{i:05d}_Dress_{i:06d}_0"
        keys.append(key)
        sg = root.require_group("samples").require_group(key)
        attrs = {"scale": 1.0 + 0.1 * i, "sample_id": f"{i:05d}_Dress", "garment_name": "Dress"}
        if grips:
            attrs["grip_vertex_idx"] = (3 * i + 1) % len(nocs)
        sg.put_attrs(attrs)
        mesh = sg.require_group("mesh")
        mesh.array("cloth_nocs_verts", np.asarray(nocs, dtype=np.float32))
        mesh.array("cloth_faces_tri", np.asarray(faces, dtype=np.int32))
    return keys
