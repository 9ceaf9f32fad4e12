"""Garments, states and plain restatements shared by tests/test_cloth_face_host.py and tests/test_gpu_cloth_face.py (the vertex-face contacts of
garmentnets_amd/cloth.py).  Every test passes its parameters explicitly: none depends on a default of cloth.py."""
import dataclasses

import numpy as np

import cloth_collision_cases as CC
from cloth_cases import sheet
from garmentnets_amd import cloth


def params(t=1.5 * CC.CELL, margin=None, R=2, K=64, relax=1.0, tf=CC.CELL, Kf=32, **kw):
    """the shared case's parameters with face contacts of thickness tf (0: off)"""
    col = dict(collision_thickness=t, collision_margin=t if margin is None else margin, collision_rebuild=R, collision_max_list=K, collision_relax=relax,
               face_thickness=tf, face_max_list=Kf)
    return cloth.ClothParams(**dict(CC.BASE, **kw), **col)


def with_constants(g, **kw):
    """g with other collision and face-contact parameters (the mesh, the masses and the constraints are not touched)"""
    p = params(**kw)
    return dataclasses.replace(g, collision=cloth.collision_constants(p), face_collision=cloth.face_collision_constants(p))


def strip(**kw):
    """the folding strip of cloth_collision_cases with face contacts on"""
    X, faces = sheet(41, 5, seed=3, size=0.8, jitter=0.1, flat=True)
    return cloth.garment(X, faces, CC.STRIP_GRIP, params(**kw))


# ------------------------------------------------------------------------------------------------ the dart
T_F = 0.01
DART_X = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.31, 0.32, 0.05], [0.36, 0.33, 0.05], [0.33, 0.37, 0.05]])
DART_FACES = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
DART_H = 1.0 / 1200.0


def dart_params(tf=T_F, R=2, relax=1.0, Kf=32):
    """no gravity, no damping, t = margin = 0.01"""
    return cloth.ClothParams(gravity=0.0, h=DART_H, damping=0.0, alpha_stretch=0.0, alpha_bend=0.05, density=0.2, collision_thickness=0.01,
                             collision_margin=0.01, collision_rebuild=R, collision_max_list=64, collision_relax=relax, face_thickness=tf,
                             face_max_list=Kf)


def dart(faces=DART_FACES, check=True, **kw):
    """one garment of two components: a big face held at vertex 0 and a small dart above it -> (garment, the start velocities: the dart falls at
    0.5 m/s, h * 0.5 = T_F / 24 a substep)"""
    v = np.zeros_like(DART_X)
    v[3:, 2] = -0.5
    return cloth.garment(DART_X, faces, 0, dart_params(**kw), check=check), v


# ------------------------------------------------------------------------------------------------ the plain restatement
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _rcp(x):
    return 1.0 / x if x > 0.0 else 0.0


def _seg(w, e, wd, inv):
    t = min(max(wd * inv, 0.0), 1.0)
    r = [w[k] - t * e[k] for k in range(3)]
    return _dot(r, r)


def plain_d2(q, a, b, c):
    """the squared distance of the definition from q to the triangle (a, b, c), python floats, one pair"""
    q, a, b, c = ([float(v) for v in p] for p in (q, a, b, c))
    e0, e1, e2 = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)], [c[k] - b[k] for k in range(3)]
    ga, gb, gc, l2 = _dot(e0, e0), _dot(e0, e1), _dot(e1, e1), _dot(e2, e2)
    idet, ia, ic, ie2 = _rcp(ga * gc - gb * gb), _rcp(ga), _rcp(gc), _rcp(l2)
    w = [q[k] - a[k] for k in range(3)]
    d0, d1 = _dot(w, e0), _dot(w, e1)
    u = [q[k] - b[k] for k in range(3)]
    seg = min(min(_seg(w, e0, d0, ia), _seg(w, e1, d1, ic)), _seg(u, e2, _dot(u, e2), ie2))
    s, t = (gc * d0 - gb * d1) * idet, (ga * d1 - gb * d0) * idet
    r = [(w[k] - s * e0[k]) - t * e1[k] for k in range(3)]
    inside = idet > 0.0 and s >= 0.0 and t >= 0.0 and s + t <= 1.0
    return min(_dot(r, r), seg) if inside else seg


def plain_face_lists(g, x):
    """the face-contact lists of the definition as a plain double loop over python floats -> [[(f, tm2)]], uncut"""
    tf2, rf2 = g.face_collision["tf2"], g.face_collision["rf2"]
    faces = np.asarray(g.faces).tolist()
    rows = []
    for i in range(len(x)):
        row = []
        for f, (a, b, c) in enumerate(faces):
            if i in (a, b, c):
                continue
            tm2 = min(tf2, plain_d2(g.x0[i], g.x0[a], g.x0[b], g.x0[c]))
            if plain_d2(x[i], x[a], x[b], x[c]) <= rf2 and tm2 > 0:
                row.append((f, tm2))
        rows.append(row)
    return rows


def assert_face_lists_are_plain(g, x, got, tag=""):
    """got = ((idx, tm2), counts, overflow) as numpy arrays against plain_face_lists, cut to Kf: indices, tm2 bits, counts, overflow, the rows' fill"""
    (idx, tm2), counts, overflow = got
    K = g.face_collision["Kf"]
    assert idx.shape == tm2.shape == (len(x), K) and idx.dtype == np.int32 and tm2.dtype == np.float64, tag
    rows = plain_face_lists(g, x)
    for i, row in enumerate(rows):
        n = min(len(row), K)
        assert counts[i] == n and overflow[i] == len(row) - n, (tag, i, counts[i], overflow[i], len(row))
        assert idx[i, :n].tolist() == [f for f, _ in row[:n]], (tag, i)
        assert tm2[i, :n].tolist() == [t for _, t in row[:n]], (tag, i)
        assert (idx[i, n:] == -1).all() and (tm2[i, n:] == 0).all(), (tag, i)
    return rows


# ------------------------------------------------------------------------------------------------ list cases
def mesh_with_points(X, faces, grip=0, **kw):
    return cloth.garment(np.asarray(X, dtype=np.float64), np.asarray(faces, dtype=np.int32), grip, params(**kw))


def at_rf():
    """a face in the plane z = 0 and loose vertices above it: vertex 3 exactly at rf (rf2 == 1.0: in the list), vertex 4 one ulp beyond (out), vertex 5
    beyond a corner at exactly rf, vertex 6 over an edge -> (garment, x)"""
    X = [[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0, np.nextafter(1.0, 2.0)], [-1.0, 0.0, 0.0], [2.0, -0.5, 0.5]]
    g = mesh_with_points(X, [[0, 1, 2]], t=0.75, margin=0.25, tf=0.75)
    assert g.face_collision["rf2"] == 1.0
    return g, g.x0.copy()


def own_corner():
    """a triangle whose corner v2 has a positive squared distance to its own face in the arithmetic of the definition (searched with the restatement;
    the test asserts that first), and a second face at the same vertices shifted a little -> (garment, x, the corner's d2 to its own face)"""
    rng = np.random.default_rng(11)
    for _ in range(2000):
        tri = rng.uniform(-1.0, 1.0, (3, 3))
        d2 = float(cloth.point_triangle(tri[2], tri[0], tri[1], tri[2])[0])
        if d2 > 0:
            break
    X = np.concatenate([tri, tri + np.array([0.0, 0.0, 0.02])])
    g = mesh_with_points(X, [[0, 1, 2], [3, 4, 5]], t=0.05, margin=0.05, tf=0.05)
    return g, g.x0.copy(), d2


def coincident_at_rest():
    """vertex 3 lies in the face's plane inside the face at rest (rest d2 == 0: excluded whatever the state), vertex 4 does not; the state lifts both
    to the same small height -> (garment, x)"""
    X = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, 0.25, 0.0], [0.5, 0.25, 0.03]]
    g = mesh_with_points(X, [[0, 1, 2]], t=0.05, margin=0.05, tf=0.05)
    x = g.x0.copy()
    x[3, 2] = x[4, 2] = 0.01
    return g, x


def stacked(Kf=3):
    """five parallel faces stacked 0.01 apart and a loose vertex above their middle, within rf of all of them: Kf = 3 keeps faces 0, 1, 2 and counts
    two -> (garment, x)"""
    X, faces = [], []
    for k in range(5):
        z = 0.01 * k
        X += [[0.0, 0.0, z], [1.0, 0.0, z], [0.0, 1.0, z]]
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
    X.append([0.25, 0.25, 0.06])
    g = mesh_with_points(X, faces, t=0.05, margin=0.05, tf=0.05, Kf=Kf)
    return g, g.x0.copy()


def bent_sheet(n=6, m=14, substeps=30, **kw):
    """an n x m sheet (6 x 14: 84 vertices, no multiple of 64, and 130 faces, one tile of 128 and two more) after a few substeps under gravity, with a
    face thickness of about a cell so that every vertex has faces it is no corner of within rf -> (garment, x)"""
    X, faces = sheet(n, m, seed=12)
    g = cloth.garment(X, faces, 30, params(t=0.06, margin=0.05, tf=0.04, **kw))
    return g, cloth.simulate_reference(dataclasses.replace(g, collision=None, face_collision=None), substeps)[0]


def list_cases():
    """name -> (garment, x): the list cases of the host tests, which the device repeats"""
    out = {"at_rf": at_rf(), "own_corner": own_corner()[:2], "coincident_at_rest": coincident_at_rest(), "stacked_K3": stacked(3), "stacked": stacked(32)}
    return out
