"""Host side of the hanging garment (no GPU): the topology, the colouring and the numpy restatement of garmentnets_amd/cloth.py against what the
definition (DESIGN.md "Hanging garments") must give, and `python -m garmentnets_amd.simulate --backend numpy` on a store that holds canonical meshes
and nothing else.  tests/test_gpu_cloth.py holds the device to this restatement bit for bit.

The bounds:
  rest length   |len - l0| <= 8 eps max(l0, |p_i|, |p_j|), eps = 2^-52, for the constraints of the LAST colour after a substep with compliance 0: nothing
                moves their vertices afterwards.  Derivation, u = eps / 2 the unit roundoff, M that maximum.  In exact arithmetic the projection leaves
                d' = d - (len - l0) n = l0 n.  Three roundings stand between that and the stored positions: (1) `len` is the square root of a three-term
                sum of squares, off by at most 2.5 u relatively, and n = d / len adds u: |n| = 1 +- 3.5 u, so the new length is l0 (1 +- 3.5 u);
                (2) the corrections (w dl) n carry the roundings of len - l0, s, the division and two products, 7 u relative to a correction of size at
                most |len - l0|, which here is below l0 / 2 (a substep from rest moves a vertex by g h^2, far less than an edge): 3.5 u l0 for the two
                ends together; (3) the additions into p_i and p_j round to u |p| per end: 2 u M.  Measuring the length again costs 2.5 u l0.  Together
                at most (3.5 + 3.5 + 2 + 2.5) u M = 5.75 eps M <= 8 eps M.
  hanging       the centroid of a corner-pinned sheet ends below -0.5 |centroid_rest - X_g|: a rigid body pinned there hangs its centroid at -1.0 times that
                distance; cloth folds, so half of it is the cap (a cap, not a measurement).
"""
import dataclasses

import numpy as np
import pytest

from cloth_cases import (EPS, FAN, PARAMS, TRIANGLE, TWO_TRIANGLES, garment, python_first_fit, sheet, sheet_counts, with_coincident, with_massless,
                         write_canonical_store)
from garmentnets_amd import cloth
from garmentnets_amd import simulate as SIM
from garmentnets_amd.io import zarr_store
from test_winding_host import open_box_mesh


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ topology
def test_single_triangle_has_three_stretch_and_no_bend():
    s, b = cloth.constraint_pairs(TRIANGLE[1])
    assert s.tolist() == [[0, 1], [0, 2], [1, 2]] and len(b) == 0


def test_two_triangles_share_one_bend():
    s, b = cloth.constraint_pairs(TWO_TRIANGLES[1])
    assert s.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]] and b.tolist() == [[0, 3]]


@pytest.mark.parametrize("n,m", [(2, 2), (5, 4), (9, 7), (3, 11)])
def test_sheet_counts_follow_the_formula(n, m):
    s, b = cloth.constraint_pairs(sheet(n, m)[1])
    assert (len(s), len(b)) == sheet_counts(n, m)
    assert (s[:, 0] < s[:, 1]).all() and (b[:, 0] < b[:, 1]).all()
    for p in (s, b):                                                 # sorted lexicographically
        assert p.tolist() == sorted(p.tolist())
    topo = cloth.topology(sheet(n, m)[1])
    assert (topo.n_stretch, topo.n_bend) == sheet_counts(n, m) and len(topo.pairs) == sum(sheet_counts(n, m))


def test_an_edge_of_three_faces_gets_no_bend():
    s, b = cloth.constraint_pairs(FAN[1])
    assert len(s) == 7 and len(b) == 0


@pytest.mark.parametrize("mesh", [TRIANGLE, TWO_TRIANGLES, FAN, sheet(5, 4), sheet(9, 7)], ids=["triangle", "two", "fan", "5x4", "9x7"])
def test_colouring_is_proper_and_is_first_fit(mesh):
    s, b = cloth.constraint_pairs(mesh[1])
    listed = np.concatenate([s, b])
    colour = cloth.first_fit_colours(listed)
    assert colour.tolist() == python_first_fit(listed.tolist())
    topo = cloth.topology(mesh[1])
    order = np.argsort(colour, kind="stable")                       # grouped by colour with a stable sort
    assert np.array_equal(topo.pairs, listed[order]) and np.array_equal(topo.is_bend, (np.arange(len(listed)) >= len(s))[order])
    assert topo.colour_off[0] == 0 and topo.colour_off[-1] == len(listed) and (np.diff(topo.colour_off) > 0).all()
    for k in range(len(topo.colour_off) - 1):
        ends = topo.pairs[topo.colour_off[k]:topo.colour_off[k + 1]].ravel()
        assert len(np.unique(ends)) == len(ends), f"colour {k}: two constraints share a vertex"
    assert cloth.topology(mesh[1].copy()) is topo                   # cached by the faces array


def test_masses_are_lumped_face_areas():
    X, faces = sheet(5, 4, seed=3)
    g = garment((X, faces), grip=6)
    area = 0.5 * np.linalg.norm(np.cross(X[faces[:, 1]] - X[faces[:, 0]], X[faces[:, 2]] - X[faces[:, 0]]), axis=1)
    mass = np.zeros(len(X))
    for f, a in zip(faces, area):
        mass[f] += PARAMS.density * a / 3
    live = np.arange(len(X)) != 6
    assert g.w[6] == 0 and np.allclose(g.w[live], 1 / mass[live], rtol=1e-13) and g.n_massless == 0
    assert np.array_equal(g.x0[6], np.zeros(3)) and np.allclose(g.x0, X - X[6], atol=0, rtol=0)
    assert np.allclose(g.l0, np.linalg.norm(X[g.pairs[:, 0]] - X[g.pairs[:, 1]], axis=1), rtol=1e-13)


def test_refusals():
    X, faces = sheet(3, 3)
    with pytest.raises(ValueError, match="grip vertex 9"):
        cloth.garment(X, faces, 9, PARAMS)
    bad = faces.copy()
    bad[2, 1] = 9
    with pytest.raises(IndexError):
        cloth.garment(X, bad, 0, PARAMS)
    with pytest.raises(IndexError):
        cloth.simulate_reference(cloth.garment(X, bad, 0, PARAMS, check=False), 1)
    with pytest.raises(ValueError, match="not finite"):
        cloth.garment(np.where(np.arange(27).reshape(9, 3) == 4, np.nan, X), faces, 0, PARAMS)
    g = garment((X, faces))
    with pytest.raises(ValueError, match="not finite"):
        cloth.simulate_reference(g, 1, x=np.where(g.x0 == g.x0[3], np.inf, g.x0))
    with pytest.raises(ValueError):
        cloth.ClothParams(h=0.0)


# ------------------------------------------------------------------------------------------------ exact statements
@pytest.mark.parametrize("substeps", [1, 7, 60])
def test_the_grip_vertex_stays_at_the_origin(substeps):
    g = garment(sheet(5, 4, seed=4), grip=9)
    x, v = cloth.simulate_reference(g, substeps)
    assert np.array_equal(bits(x[9]), bits(np.zeros(3))) and np.array_equal(bits(v[9]), bits(np.zeros(3)))
    assert np.abs(x - g.x0).max() > 1e-6                             # the rest moved


def test_without_gravity_nothing_moves():
    g = garment(sheet(9, 7, seed=5), grip=11, params=dataclasses.replace(PARAMS, gravity=0.0))
    x, v = cloth.simulate_reference(g, 25)
    assert np.array_equal(bits(x), bits(g.x0)) and not v.any()


def test_a_massless_vertex_stays_where_it_started():
    X, faces, lone = with_massless()
    g = garment((X, faces), grip=2)
    assert g.n_massless == 2 and all(g.w[k] == 0 for k in lone)
    x, v = cloth.simulate_reference(g, 40)
    for k in lone:
        assert np.array_equal(bits(x[k]), bits(g.x0[k])) and not v[k].any()
    assert np.isfinite(x).all() and np.abs(x - g.x0).max() > 1e-4
    assert cloth.diagnostics(g, x, v)["massless_vertices"] == 2


def test_zero_length_and_zero_weight_constraints_change_nothing():
    p = np.array([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.5, 0.5, 0.5], [0.0, 0.0, 1.0]])
    w = np.array([2.0, 3.0, 0.0, 0.0, 1.0, 1.0])
    before = p.copy()
    # (0, 1): len == 0; (2, 3): w_i + w_j + alpha_t == 0; (4, 5): an ordinary one, which must move
    cloth.project_colour(p, w, np.array([0, 2, 4]), np.array([1, 3, 5]), np.array([0.5, 1.0, 0.2]), np.array([0.0, 0.0, 0.0]))
    assert np.array_equal(bits(p[:4]), bits(before[:4])) and np.isfinite(p).all()
    assert abs(np.linalg.norm(p[4] - p[5]) - 0.2) < 1e-15 and not np.array_equal(p[4:], before[4:])
    # and through a whole run: coincident vertices (len == 0 from the first substep on), two held ends of one stretch constraint (s == 0)
    g = garment(with_coincident(), grip=0, params=dataclasses.replace(PARAMS, alpha_stretch=0.0))
    c = int(np.flatnonzero((g.pairs == [6, 7]).all(axis=1))[0])
    assert g.l0[c] == 0
    w2 = g.w.copy()
    w2[[12, 13]] = 0.0
    g2 = dataclasses.replace(g, w=w2)
    assert ((g2.w[g2.pairs[:, 0]] + g2.w[g2.pairs[:, 1]] + g2.alpha_t) == 0).any()
    x, v = cloth.simulate_reference(g2, 50)
    assert np.isfinite(x).all() and np.isfinite(v).all()
    assert np.array_equal(bits(x[[12, 13]]), bits(g.x0[[12, 13]])) and np.abs(x - g.x0).max() > 1e-4


def test_the_order_inside_a_colour_changes_no_bit():
    g = garment(sheet(9, 7, seed=6), grip=30)
    rng = np.random.default_rng(0)
    perm = np.concatenate([g.colour_off[k] + rng.permutation(g.colour_off[k + 1] - g.colour_off[k]) for k in range(len(g.colour_off) - 1)])
    assert not np.array_equal(perm, np.arange(len(perm)))
    g2 = dataclasses.replace(g, pairs=g.pairs[perm], is_bend=g.is_bend[perm], l0=g.l0[perm], alpha_t=g.alpha_t[perm])
    a, b = cloth.simulate_reference(g, 30), cloth.simulate_reference(g2, 30)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def test_two_hundred_substeps_equal_four_times_fifty():
    g = garment(sheet(5, 4, seed=7), grip=3)
    whole = cloth.simulate_reference(g, 200)
    x = v = None
    for _ in range(4):
        x, v = cloth.simulate_reference(g, 50, x, v)
    assert np.array_equal(bits(whole[0]), bits(x)) and np.array_equal(bits(whole[1]), bits(v))


# ------------------------------------------------------------------------------------------------ a derived bound
@pytest.mark.parametrize("substeps", [1, 20])
def test_the_last_colour_ends_a_substep_at_its_rest_lengths(substeps):
    """the module docstring derives the bound; with both compliances 0 it holds for the bend constraints of the last colour as for the stretch ones"""
    checked = 0
    for name, mesh, grip in (("triangle", TRIANGLE, 0), ("two", TWO_TRIANGLES, 1), ("5x4", sheet(5, 4, seed=8), 0), ("9x7", sheet(9, 7, seed=9), 20)):
        g = garment(mesh, grip=grip, params=dataclasses.replace(PARAMS, h=1.0 / 2000.0, alpha_stretch=0.0, alpha_bend=0.0))
        x, _ = cloth.simulate_reference(g, substeps)
        last = slice(g.colour_off[-2], g.colour_off[-1])
        i, j, l0 = g.pairs[last, 0], g.pairs[last, 1], g.l0[last]
        d = x[i] - x[j]
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        M = np.maximum(l0, np.maximum(np.linalg.norm(x[i], axis=1), np.linalg.norm(x[j], axis=1)))
        worst = float((np.abs(length - l0) / (EPS * M)).max())
        n_stretch = int((~g.is_bend[last]).sum())
        print(f"[cloth] {name}, {substeps} substeps: last colour {len(l0)} constraints ({n_stretch} stretch), |len - l0| <= {worst:.2f} eps M (bound 8)")
        assert (np.abs(length - l0) <= 8 * EPS * M).all()
        checked += n_stretch
    assert checked > 0                                               # the statement about STRETCH constraints is not vacuous


# ------------------------------------------------------------------------------------------------ a loose physical condition
def test_a_corner_pinned_sheet_hangs():
    X, faces = sheet(12, 12, seed=10, size=0.3, jitter=0.1, flat=True)
    assert not X[:, 2].any()                                         # started horizontally
    params = cloth.ClothParams(gravity=9.81, h=1.0 / 600.0, damping=3.0, alpha_stretch=0.0, alpha_bend=0.05, density=0.2)
    g = cloth.garment(X, faces, 0, params)
    x, v = cloth.simulate_reference(g, 1500)                         # 2.5 s
    arm = float(np.linalg.norm(g.x0.mean(axis=0)))                   # |centroid_rest - X_g|: the grip is the origin
    diag = cloth.diagnostics(g, x, v)
    print(f"[cloth] corner-pinned 12 x 12 sheet after 2.5 s: centroid z {x.mean(axis=0)[2]:.4f} (cap {-0.5 * arm:.4f}, rigid {-arm:.4f}), "
          f"largest stretch strain {diag['max_stretch_strain']:.4f}, kinetic energy {diag['kinetic_energy']:.3e} J")
    assert x.mean(axis=0)[2] < -0.5 * arm
    assert np.array_equal(bits(x[0]), bits(np.zeros(3)))


# ------------------------------------------------------------------------------------------------ python -m garmentnets_amd.simulate
SIM_FLAGS = ["--backend", "numpy", "--h", "0.004", "--duration", "0.1", "--damping", "1.0", "--alpha_stretch", "0", "--alpha_bend", "0.01", "--density", "0.25",
             "--gravity", "9.81"]


def box(seed, n=2):
    return open_box_mesh(seed, n=n)


def test_simulate_writes_cloth_verts_attributes_and_summary(tmp_path):
    store = str(tmp_path / "d.zarr")
    meshes = [box(0), box(1, n=3)]
    keys = write_canonical_store(store, meshes)
    out = SIM.main(["--zarr_in", store] + SIM_FLAGS)
    assert out["samples"] == 2 and out["written"] == 2 and out["substeps"] == 25 and out["summary_written"]
    root = zarr_store.open_group(store, create=False)
    params = cloth.ClothParams(gravity=9.81, h=0.004, damping=1.0, alpha_stretch=0.0, alpha_bend=0.01, density=0.25)
    boxes = []
    for i, (key, (nocs, faces)) in enumerate(zip(keys, meshes)):
        mesh = root["samples"][key]["mesh"]
        got = mesh["cloth_verts"][:]
        grip = (3 * i + 1) % len(nocs)
        g = cloth.garment_from_nocs(np.asarray(nocs, np.float32), faces, grip, cloth.rest_scale_of(root["summary"]["cloth_canonical_aabb_union"][:]), params)
        x, v = cloth.simulate_reference(g, 25)
        assert got.dtype == np.float32 and np.array_equal(got, x.astype(np.float32)) and not got[grip].any()
        rec = mesh.attrs["cloth_simulation"]
        assert rec["substeps"] == 25 and rec["h"] == 0.004 and rec["density"] == 0.25 and rec["grip_vertex_idx"] == grip and rec["massless_vertices"] == 0
        assert rec["kinetic_energy"] == cloth.diagnostics(g, x, v)["kinetic_energy"] > 0 and rec["max_stretch_strain"] >= 0
        boxes.append(got)
    union = root["summary"]["cloth_aabb_union"][:]
    assert union.dtype == np.float32 and np.array_equal(union, np.stack([np.min([b.min(0) for b in boxes], 0), np.max([b.max(0) for b in boxes], 0)]))


def test_simulate_keeps_what_is_there_unless_told_to_overwrite(tmp_path):
    store = str(tmp_path / "d.zarr")
    keys = write_canonical_store(store, [box(2), box(3)])
    SIM.main(["--zarr_in", store] + SIM_FLAGS)
    root = zarr_store.open_group(store, create=False)
    first = [root["samples"][k]["mesh"]["cloth_verts"][:] for k in keys]
    union = root["summary"]["cloth_aabb_union"][:]
    longer = SIM_FLAGS[:SIM_FLAGS.index("--duration") + 1] + ["0.2"] + SIM_FLAGS[SIM_FLAGS.index("--duration") + 2:]
    out = SIM.main(["--zarr_in", store] + longer)
    assert out["written"] == 0 and not out["summary_written"]
    assert all(np.array_equal(root["samples"][k]["mesh"]["cloth_verts"][:], a) for k, a in zip(keys, first))
    out = SIM.main(["--zarr_in", store, "--overwrite"] + longer)
    assert out["written"] == 2 and out["substeps"] == 50 and not out["summary_written"]
    assert all(not np.array_equal(root["samples"][k]["mesh"]["cloth_verts"][:], a) for k, a in zip(keys, first))
    assert root["samples"][keys[0]]["mesh"].attrs["cloth_simulation"]["substeps"] == 50
    assert np.array_equal(root["summary"]["cloth_aabb_union"][:], union)          # kept: the store had one
    out = SIM.main(["--zarr_in", store, "--update_summary"] + longer)
    assert out["written"] == 0 and out["summary_written"] and not np.array_equal(root["summary"]["cloth_aabb_union"][:], union)


def test_a_drawn_grip_is_reproducible_from_the_seed(tmp_path):
    meshes = [box(4), box(5, n=3), box(6)]
    grips = {}
    for name, seed in (("a", 11), ("b", 11), ("c", 12)):
        store = str(tmp_path / f"{name}.zarr")
        keys = write_canonical_store(store, meshes, grips=False, canonical_aabb=False)
        with pytest.raises(SystemExit):                              # no canonical box and no --rest_scale
            SIM.main(["--zarr_in", store] + SIM_FLAGS)
        SIM.main(["--zarr_in", store, "--seed", str(seed), "--rest_scale", "0.8"] + SIM_FLAGS)
        samples = zarr_store.open_group(store, create=False)["samples"]
        grips[name] = [samples[k].attrs["grip_vertex_idx"] for k in keys]
        for i, k in enumerate(keys):
            assert grips[name][i] == int(np.random.RandomState(seed + i).randint(0, len(meshes[i][0])))
            assert not samples[k]["mesh"]["cloth_verts"][:][grips[name][i]].any()
            assert samples[k]["mesh"].attrs["cloth_simulation"]["rest_scale"] == 0.8
    assert grips["a"] == grips["b"] != grips["c"]
