"""Garments, states and plain restatements shared by tests/test_cloth_collision_host.py and tests/test_gpu_cloth_collision.py (the self-collision of
garmentnets_amd/cloth.py).  Every test passes its parameters explicitly: none depends on a default of cloth.py."""
import dataclasses

import numpy as np

from cloth_cases import TRIANGLE, sheet
from garmentnets_amd import cloth

CELL = 0.02                                                          # the strip's cell: 0.8 / 40
BASE = dict(gravity=9.81, h=1.0 / 1200.0, damping=2.0, alpha_stretch=0.0, alpha_bend=0.05, density=0.2)
STRIP_GRIP = 102                                                     # row 20, column 2
LEFT, RIGHT = np.arange(0, 16 * 5), np.arange(25 * 5, 41 * 5)        # the vertices of rows 0-15 and of rows 25-40


def params(t=1.5 * CELL, margin=None, R=2, K=64, relax=1.0, **kw):
    """the shared case's parameters; t = 0: contacts off"""
    col = {} if t == 0 else dict(collision_thickness=t, collision_margin=t if margin is None else margin, collision_rebuild=R, collision_max_list=K,
                                 collision_relax=relax)
    return cloth.ClothParams(**dict(BASE, **kw), **col)


def strip(**kw):
    """the folding strip: a flat 41 x 5 sheet held at its centre, so its two halves swing together"""
    X, faces = sheet(41, 5, seed=3, size=0.8, jitter=0.1, flat=True)
    return cloth.garment(X, faces, STRIP_GRIP, params(**kw))


def with_constants(g, **kw):
    """g with other collision parameters (the mesh, the masses and the constraints are not touched)"""
    return dataclasses.replace(g, collision=cloth.collision_constants(params(**kw)))


def points(X, grip=0, **kw):
    """a garment of loose vertices (no face: every w is 0): only its contact lists are of interest"""
    return cloth.garment(np.asarray(X, dtype=np.float64), np.zeros((0, 3), dtype=np.int32), grip, params(**kw))


def triangle(**kw):
    return cloth.garment(TRIANGLE[0], TRIANGLE[1], 0, params(**kw))


def sq(a, b):
    dx, dy, dz = float(a[0]) - float(b[0]), float(a[1]) - float(b[1]), float(a[2]) - float(b[2])
    return (dx * dx + dy * dy) + dz * dz


def plain_lists(g, x):
    """the contact lists of the definition as a plain double loop over python floats -> [[(j, tm2)]], uncut"""
    t2, r2 = g.collision["t2"], g.collision["r2"]
    rows = []
    for i in range(len(x)):
        row = []
        for j in range(len(x)):
            if j == i:
                continue
            tm2 = min(t2, sq(g.x0[i], g.x0[j]))
            if sq(x[i], x[j]) <= r2 and tm2 > 0:
                row.append((j, tm2))
        rows.append(row)
    return rows


def assert_lists_are_plain(g, x, got, tag=""):
    """got = ((idx, tm2), counts, overflow) as numpy arrays against plain_lists, cut to K: indices, tm2 bits, counts, overflow, the fill of the rows"""
    (idx, tm2), counts, overflow = got
    K = g.collision["K"]
    assert idx.shape == tm2.shape == (len(x), K) and idx.dtype == np.int32 and tm2.dtype == np.float64, tag
    for i, row in enumerate(plain_lists(g, x)):
        n = min(len(row), K)
        assert counts[i] == n and overflow[i] == len(row) - n, (tag, i, counts[i], overflow[i], len(row))
        assert idx[i, :n].tolist() == [j for j, _ in row[:n]], (tag, i)
        assert tm2[i, :n].tolist() == [t for _, t in row[:n]], (tag, i)
        assert (idx[i, n:] == -1).all() and (tm2[i, n:] == 0).all(), (tag, i)


def packed(n=70, seed=5, **kw):
    """n loose vertices inside a cube of edge r / 4 (one cell or two, every pair within r), vertex 5 on vertex 4 at rest: that pair is excluded, every
    other vertex has n - 1 partners -- a bucket longer than a wave and lists longer than K"""
    r = cloth.collision_constants(params(**kw))["r"]
    X = np.random.default_rng(seed).uniform(0.1 * r, 0.35 * r, (n, 3))
    X[5] = X[4]
    return points(X, **kw)


def on_borders(**kw):
    """loose vertices on and beside the borders of the grid's cells, on both sides of the origin -> (garment, x): the start pose is a jittered lattice
    (every rest distance positive), the state puts vertices exactly on multiples of the cell edge, one ulp beside them and in between"""
    from garmentnets_amd import ops
    g0 = points(np.zeros((1, 3)), **kw)
    cell = ops.cloth_collision_constants([g0], "test")["cell"]
    ticks = []
    for k in (-2.0, -1.0, 0.0, 1.0, 2.0):
        ticks += [np.nextafter(k * cell, -np.inf), k * cell, np.nextafter(k * cell, np.inf), (k + 0.5) * cell]
    ticks = np.array(ticks)
    rng = np.random.default_rng(9)
    x = np.stack([rng.choice(ticks, 150), rng.choice(ticks, 150), rng.choice(ticks[:8], 150)], axis=1)
    X = rng.uniform(-1.0, 1.0, x.shape)
    return points(X, **kw), x
