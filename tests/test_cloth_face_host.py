"""The vertex-face contacts of garmentnets_amd/cloth.py held to their definition, without a GPU: point_triangle against distance.py's squared
distance (bit for bit) and region by region, the face-contact lists against a plain double loop over python floats, the exact properties of the
solver with face entries, the dart that falls through a face without them, and `simulate --face_contacts` with the numpy backend.
tests/test_gpu_cloth_face.py holds the device to this restatement."""
import dataclasses
import json

import numpy as np
import pytest

import cloth_collision_cases as CC
import cloth_face_cases as FC
from cloth_cases import write_canonical_store
from garmentnets_amd import cloth, distance
from garmentnets_amd import simulate as SIM
from garmentnets_amd.io import zarr_store
from test_winding_host import open_box_mesh

ONE_FACE = np.array([[0, 1, 2]], dtype=np.int32)


def reference_d2(q, tri):
    return np.array([distance.point_mesh_sqdist_reference(q[k:k + 1], tri[k], ONE_FACE)[1][0] for k in range(len(q))])


def region_points(tri, rng, n=8):
    """points over the interior, over each edge and beyond each corner of the triangle tri (3, 3), lifted off its plane -> {region: (n, 3)}"""
    a, b, c = tri
    nrm = np.cross(b - a, c - a)
    nrm = nrm / np.linalg.norm(nrm)
    lift = rng.uniform(-0.5, 0.5, (n, 1)) * nrm
    out = {}
    u = rng.uniform(0.1, 0.4, (n, 2))
    out["interior"] = a + u[:, :1] * (b - a) + u[:, 1:] * (c - a) + lift
    for name, (p, q, r) in {"edge01": (a, b, c), "edge02": (a, c, b), "edge12": (b, c, a)}.items():
        t = rng.uniform(0.2, 0.8, (n, 1))
        foot = p + t * (q - p)
        away = foot - r                                           # from the opposite corner through the edge: outside, over this edge
        away = away - ((away * (q - p)).sum(1, keepdims=True) / ((q - p) ** 2).sum()) * (q - p)
        out[name] = foot + rng.uniform(0.2, 0.6, (n, 1)) * away / np.linalg.norm(away, axis=1, keepdims=True) + lift
    centre = (a + b + c) / 3.0
    for name, p in {"corner0": a, "corner1": b, "corner2": c}.items():
        out[name] = p + rng.uniform(0.3, 0.8, (n, 1)) * (p - centre) + lift
    return out


# ------------------------------------------------------------------------------------------------ point_triangle
def test_point_triangle_d2_is_the_distance_reference_bit_for_bit():
    rng = np.random.default_rng(0)
    tri = rng.normal(size=(300, 3, 3))
    q = rng.normal(size=(300, 3))
    d2 = cloth.point_triangle(q, tri[:, 0], tri[:, 1], tri[:, 2])[0]
    assert d2.dtype == np.float64 and np.array_equal(d2, reference_d2(q, tri))
    # region by region on one triangle
    one = np.array([[0.1, -0.2, 0.05], [0.9, 0.1, -0.1], [0.2, 0.8, 0.3]])
    for name, pts in region_points(one, rng).items():
        t = np.broadcast_to(one, (len(pts), 3, 3))
        assert np.array_equal(cloth.point_triangle(pts, one[0], one[1], one[2])[0], reference_d2(pts, t)), name
    # a zero-area triangle (three collinear points, and three coincident ones) and a sliver
    flat = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25], [2.0, 1.0, 0.5]])
    point = np.array([[0.3, 0.3, 0.3]] * 3)
    sliver = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1e-9, 0.0]])
    for name, t in (("collinear", flat), ("coincident", point), ("sliver", sliver)):
        pts = rng.normal(size=(64, 3))
        tt = np.broadcast_to(t, (64, 3, 3))
        d2, r, bary = cloth.point_triangle(pts, t[0], t[1], t[2])
        assert np.array_equal(d2, reference_d2(pts, tt)), name
        assert np.isfinite(r).all() and np.isfinite(bary).all() and (bary >= 0).all() and (bary <= 1).all(), name


def test_point_triangle_weights_in_every_region():
    """bary has its zeros where the region says, lies in [0, 1], and rebuilds the closest point q - r.  Bound: the coordinates here are below 2 in
    magnitude, the weights in [0, 1]; q - r and sum(bary_k v_k) are each a handful of fp64 operations on such numbers away from the exact closest
    point -- the weights carry a relative error of a few eps (s and t through the 2 x 2 solve of a triangle with det ~ 0.4, the segment parameters
    through one division) -- so 64 eps * 2 bounds their difference with a wide margin (a sliver, where a * c / det is large, would need that
    factor in the bound and is not measured here)."""
    eps = 2.0 ** -52
    rng = np.random.default_rng(1)
    one = np.array([[0.1, -0.2, 0.05], [0.9, 0.1, -0.1], [0.2, 0.8, 0.3]])
    zeros = {"interior": [], "edge01": [2], "edge02": [1], "edge12": [0], "corner0": [1, 2], "corner1": [0, 2], "corner2": [0, 1]}
    for name, pts in region_points(one, rng, n=16).items():
        d2, r, bary = cloth.point_triangle(pts, one[0], one[1], one[2])
        assert (bary >= 0).all() and (bary <= 1).all(), name
        for k in range(3):
            if k in zeros[name]:
                assert (bary[:, k] == 0).all(), (name, k)
            else:
                assert (bary[:, k] > 0).all(), (name, k)
        assert np.abs(bary.sum(axis=1) - 1.0).max() <= 4 * eps, name
        rebuilt = (bary[:, :, None] * one[None]).sum(axis=1)
        assert np.abs(rebuilt - (pts - r)).max() <= 64 * eps * 2.0, (name, np.abs(rebuilt - (pts - r)).max())
        assert np.array_equal(d2, (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]), name
    # at a corner exactly: the corner's weight is 1, the distance 0
    d2, r, bary = cloth.point_triangle(one[1], one[0], one[1], one[2])
    assert bary.tolist() == [0.0, 1.0, 0.0] and d2 == 0.0 and not r.any()


# ------------------------------------------------------------------------------------------------ lists
@pytest.mark.parametrize("name", ["at_rf", "own_corner", "coincident_at_rest", "stacked_K3", "stacked"])
def test_lists_are_the_plain_double_loop(name):
    g, x = FC.list_cases()[name]
    FC.assert_face_lists_are_plain(g, x, cloth.face_contact_lists_reference(g, x), name)
    FC.assert_face_lists_are_plain(g, x, cloth.face_contact_lists_reference(g, x, chunk=3), name + ", chunks of 3")


def test_a_vertex_exactly_at_rf_is_in_the_list_and_one_ulp_beyond_is_not():
    g, x = FC.at_rf()
    (idx, tm2), counts, overflow = cloth.face_contact_lists_reference(g, x)
    assert counts.tolist() == [0, 0, 0, 1, 0, 1, 1] and not overflow.any()
    assert idx[3, 0] == 0 and tm2[3, 0] == g.face_collision["tf2"] == 0.75 * 0.75 and idx[4, 0] == -1
    assert FC.plain_d2(x[3], x[0], x[1], x[2]) == 1.0 and FC.plain_d2(x[4], x[0], x[1], x[2]) > 1.0


def test_incident_faces_are_out_by_index_even_where_the_corner_has_a_positive_distance():
    g, x, d2 = FC.own_corner()
    assert d2 > 0 and float(cloth.point_triangle(g.x0[2], g.x0[0], g.x0[1], g.x0[2])[0]) > 0, "the case needs a corner off its own face"
    (idx, _), counts, _ = cloth.face_contact_lists_reference(g, x)
    assert idx[:, 0].tolist() == [1, 1, 1, 0, 0, 0] and counts.tolist() == [1] * 6


def test_a_face_coincident_with_the_vertex_at_rest_is_out():
    g, x = FC.coincident_at_rest()
    (idx, tm2), counts, _ = cloth.face_contact_lists_reference(g, x)
    assert counts.tolist() == [0, 0, 0, 0, 1] and idx[3, 0] == -1 and idx[4, 0] == 0 and 0 < tm2[4, 0] < g.face_collision["tf2"]


def test_a_cut_list_keeps_the_smallest_faces_and_counts_the_rest():
    g, x = FC.stacked(3)
    (idx, _), counts, overflow = cloth.face_contact_lists_reference(g, x)
    assert idx[15].tolist() == [0, 1, 2] and counts[15] == 3 and overflow[15] == 2
    assert idx[0].tolist() == [1, 2, 3] and overflow[0] == 1                       # face 0 is its own


# ------------------------------------------------------------------------------------------------ exact properties
def test_without_gravity_nothing_moves_and_the_grip_stays_at_the_origin():
    still = FC.strip(gravity=0.0)
    x, v, stats = cloth.simulate_reference(still, 12, stats=True)
    assert np.array_equal(x, still.x0) and not v.any() and stats["face_contact_active"] == 0 and stats["face_contact_max_list"] > 0
    g = FC.strip()
    x, v, stats = cloth.simulate_reference(g, 60, stats=True)
    assert not x[CC.STRIP_GRIP].any() and not v[CC.STRIP_GRIP].any() and np.abs(x - g.x0).max() > 1e-4
    assert set(stats) == set(cloth.CONTACT_STATS) | set(cloth.FACE_CONTACT_STATS)


def test_face_thickness_zero_is_the_run_of_today():
    off, plain = FC.strip(tf=0.0), CC.strip()
    assert off.face_collision is None and off.collision == plain.collision
    a, b = cloth.simulate_reference(off, 80, stats=True), cloth.simulate_reference(plain, 80, stats=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and tuple(a[2]) == cloth.CONTACT_STATS


def test_two_hundred_substeps_equal_four_times_fifty_at_a_rebuild_of_five():
    g = FC.bent_sheet(R=5)[0]
    want = cloth.simulate_reference(g, 200, stats=True)
    x = v = None
    sums = dict.fromkeys(("contact_active", "contact_overflow", "face_contact_active", "face_contact_overflow"), 0)
    for _ in range(4):
        x, v, s = cloth.simulate_reference(g, 50, x, v, stats=True)
        sums = {k: n + s[k] for k, n in sums.items()}
    assert np.array_equal(x, want[0]) and np.array_equal(v, want[1]) and sums == {k: want[2][k] for k in sums}
    assert want[2]["face_contact_max_list"] > 0


def test_face_entries_of_which_none_is_active_change_no_bit_of_the_vertex_entries():
    """a face thickness of a micrometre under a margin of centimetres: every vertex has face entries, none can be active"""
    thin, plain = FC.strip(tf=1e-6), CC.strip()
    warm = cloth.simulate_reference(plain, 300)
    a, b = cloth.simulate_reference(thin, 80, *warm, stats=True), cloth.simulate_reference(plain, 80, *warm, stats=True)
    assert a[2]["face_contact_max_list"] > 0 and a[2]["face_contact_active"] == 0 and b[2]["contact_active"] > 0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and {k: a[2][k] for k in cloth.CONTACT_STATS} == b[2]


# ------------------------------------------------------------------------------------------------ the scenario
def fall(g, v0, substeps=400):
    low = [np.inf]

    def observe(s, x, v):
        low[0] = min(low[0], float(x[3:, 2].min()))
    x, v, stats = cloth.simulate_reference(g, substeps, g.x0, v0, stats=True, observe=observe)
    return low[0], x, stats


def test_the_dart_is_stopped_by_the_face_with_face_contacts_and_falls_through_it_without():
    """a dart falling at 0.5 m/s (t_f / 24 a substep) onto the middle of a face a hundred times its size.  Measured: lowest height 0.99998 t_f with
    face contacts (9 active entries), -11.667 t_f (free flight) without."""
    g, v0 = FC.dart()
    low, x, stats = fall(g, v0)
    print(f"with face contacts: lowest dart height {low / FC.T_F:.5f} t_f, {stats}")
    assert low > 0.9 * FC.T_F
    assert stats["face_contact_active"] > 0
    assert np.array_equal(x[:3], g.x0[:3]), "the big face's vertices keep their bits"
    assert stats["contact_travel"] <= 1 and stats["face_contact_overflow"] == 0
    off, v0 = FC.dart(tf=0.0)
    low_off, x_off, stats_off = fall(off, v0)
    print(f"without: the dart ends at {x_off[3:, 2].max() / FC.T_F:.3f} t_f, {stats_off}")
    assert x_off[3:, 2].max() < -10 * FC.T_F
    assert np.array_equal(x_off[:3], off.x0[:3]) and stats_off["contact_travel"] <= 1 and tuple(stats_off) == cloth.CONTACT_STATS


# ------------------------------------------------------------------------------------------------ parameters
def test_parameters_and_constants():
    for kw, msg in (({"tf": -0.01}, "face_thickness must not be negative"), ({"Kf": 0}, "face_max_list"), ({"Kf": 33}, "face_max_list"),
                    ({"Kf": 2.5}, "face_max_list"), ({"tf": float("nan")}, "finite")):
        with pytest.raises(ValueError, match=msg):
            FC.params(**kw)
    with pytest.raises(ValueError, match="needs collision_thickness > 0"):
        cloth.ClothParams(face_thickness=0.01)
    c = cloth.face_collision_constants(FC.params(t=0.03, margin=0.01, tf=0.02, Kf=7))
    assert c == {"tf2": 0.02 * 0.02, "rf": 0.02 + 0.01, "rf2": (0.02 + 0.01) * (0.02 + 0.01), "Kf": 7}
    assert cloth.face_collision_constants(FC.params(tf=0.0)) is None and cloth.face_collision_constants(cloth.ClothParams()) is None
    assert cloth.FACE_COLLISION_FIELDS == ("face_thickness", "face_max_list") and cloth.FACE_MAX_LIST_CAP == 32
    assert cloth.COLLISION_FIELDS == ("collision_thickness", "collision_margin", "collision_rebuild", "collision_max_list", "collision_relax")
    assert cloth.CONTACT_STATS == ("contact_overflow", "contact_max_list", "contact_travel", "contact_active")
    assert cloth.collision_constants(FC.params()) == cloth.collision_constants(CC.params())
    g = FC.strip()
    assert g.faces.shape == (320, 3) and g.face_collision == cloth.face_collision_constants(FC.params()) and CC.strip().face_collision is None
    with pytest.raises(ValueError, match="face contacts off"):
        cloth.face_contact_lists_reference(CC.strip(), g.x0)
    with pytest.raises(ValueError, match="need the vertex contacts"):
        cloth.simulate_reference(dataclasses.replace(g, collision=None), 1)


# ------------------------------------------------------------------------------------------------ simulate
COLLISION = ["--self_collision", "--collision_thickness", "0.3", "--collision_margin", "0.1", "--collision_rebuild", "2", "--collision_max_list", "64",
             "--collision_relax", "1.0"]
FACE = ["--face_contacts", "--face_thickness", "0.1", "--face_max_list", "24"]
FLAGS = ["--h", "0.004", "--duration", "0.4", "--damping", "2", "--alpha_stretch", "0", "--alpha_bend", "0.01", "--density", "0.25", "--gravity", "9.81"]
BASE_KEYS = {"gravity", "h", "damping", "alpha_stretch", "alpha_bend", "density", "duration", "substeps", "rest_scale", "grip_vertex_idx",
             "kinetic_energy", "max_stretch_strain", "massless_vertices"}


def test_simulate_with_face_contacts_records_parameters_and_diagnostics(tmp_path, capsys):
    meshes = [open_box_mesh(0, n=3), open_box_mesh(1, n=4, drop=1)]
    plain, vert, face, tight = (str(tmp_path / f"{n}.zarr") for n in ("plain", "vert", "face", "tight"))
    for path in (plain, vert, face, tight):
        keys = write_canonical_store(path, meshes)
    SIM.main(["--zarr_in", plain, "--backend", "numpy"] + FLAGS)
    SIM.main(["--zarr_in", vert, "--backend", "numpy"] + COLLISION + FLAGS)
    out = SIM.main(["--zarr_in", face, "--backend", "numpy"] + COLLISION + FACE + FLAGS)
    assert out["written"] == 2
    a, b, c = (zarr_store.open_group(p, create=False) for p in (plain, vert, face))
    base = cloth.ClothParams(gravity=9.81, h=0.004, damping=2.0, alpha_stretch=0.0, alpha_bend=0.01, density=0.25)
    for key in keys:
        ra, rb, rc = (r["samples"][key]["mesh"].attrs["cloth_simulation"] for r in (a, b, c))
        assert set(ra) == BASE_KEYS
        assert set(rb) == BASE_KEYS | set(cloth.COLLISION_FIELDS) | set(cloth.CONTACT_STATS)
        assert set(rc) == set(rb) | set(cloth.FACE_COLLISION_FIELDS) | set(cloth.FACE_CONTACT_STATS)
        mesh = c["samples"][key]["mesh"]
        assert rc["face_thickness"] == 0.1 and rc["face_max_list"] == 24 and rc["collision_thickness"] == 0.3 and rc["collision_margin"] == 0.1
        assert {k: rb[k] for k in cloth.COLLISION_FIELDS} == {k: rc[k] for k in cloth.COLLISION_FIELDS}
        on = dataclasses.replace(base, **{k: rc[k] for k in cloth.COLLISION_FIELDS + cloth.FACE_COLLISION_FIELDS})
        want = cloth.simulate_reference(cloth.garment_from_nocs(mesh["cloth_nocs_verts"][:], mesh["cloth_faces_tri"][:], rc["grip_vertex_idx"],
                                                                rc["rest_scale"], on), 100, stats=True)
        assert np.array_equal(mesh["cloth_verts"][:], want[0].astype(np.float32))
        assert {k: rc[k] for k in cloth.CONTACT_STATS + cloth.FACE_CONTACT_STATS} == want[2]
        assert rc["face_contact_max_list"] > 0
        assert (key in out["contact_warnings"]) == (rc["contact_overflow"] > 0 or rc["contact_travel"] > 1 or rc["face_contact_overflow"] > 0)
    # a face list of one entry under a wide reach: cut lists, named in the warning with the face diagnostic
    capsys.readouterr()
    out = SIM.main(["--zarr_in", tight, "--backend", "numpy"] + COLLISION + ["--face_contacts", "--face_max_list", "1", "--face_thickness", "0.2"] + FLAGS)
    assert out["contact_warnings"] == keys
    rows = [json.loads(line) for line in capsys.readouterr().out.splitlines()]
    warnings = [r["warning"] for r in rows if "warning" in r]
    assert len(warnings) == 2 and all(k in w and "face_contact_overflow" in w and "--face_max_list" in w for k, w in zip(keys, warnings))
    recs = [zarr_store.open_group(tight, create=False)["samples"][k]["mesh"].attrs["cloth_simulation"] for k in keys]
    assert all(r["face_contact_overflow"] > 0 and r["face_max_list"] == 1 for r in recs)


def test_face_contacts_without_self_collision_is_an_argparse_error(tmp_path, capsys):
    path = str(tmp_path / "s.zarr")
    write_canonical_store(path, [open_box_mesh(0, n=3)])
    with pytest.raises(SystemExit) as e:
        SIM.main(["--zarr_in", path, "--backend", "numpy", "--face_contacts"] + FLAGS)
    assert e.value.code == 2 and "--face_contacts needs --self_collision" in capsys.readouterr().err
    assert "mesh/cloth_verts" not in zarr_store.open_group(path, create=False)["samples"][sorted(zarr_store.open_group(path, create=False)["samples"].keys())[0]]
