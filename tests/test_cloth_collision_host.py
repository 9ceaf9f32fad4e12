"""Host (no GPU): the self-collision of garmentnets_amd/cloth.py held to its definition -- the contact lists against a plain double loop, the invariants
without tolerance, the folding strip whose halves pass through each other without contacts and stay a thickness apart with them, the parameter
refusals and `simulate --backend numpy --self_collision`.  tests/test_gpu_cloth_collision.py holds the device to this restatement bit for bit."""
import dataclasses
import json

import numpy as np
import pytest

import cloth_collision_cases as CC
from cloth_cases import sheet, with_coincident, write_canonical_store
from garmentnets_amd import cloth
from garmentnets_amd import simulate as SIM
from garmentnets_amd.io import zarr_store
from test_winding_host import open_box_mesh

STATS0 = {"contact_overflow": 0, "contact_max_list": 0, "contact_travel": 0.0, "contact_active": 0}


@pytest.fixture(scope="module")
def folded():
    """the strip and its state after 384 substeps with contacts: the halves have met"""
    g = CC.strip()
    return g, cloth.simulate_reference(g, 384)


# ------------------------------------------------------------------------------------------------ lists
def test_lists_of_a_triangle_equal_a_plain_double_loop():
    g = CC.triangle(t=0.15, margin=0.08)                             # r = 0.23: the edge of 0.2009 is in, the edges of 0.2557 and 0.2627 are out
    got = cloth.contact_lists_reference(g, g.x0)
    CC.assert_lists_are_plain(g, g.x0, got, "triangle")
    assert got[1].tolist() == [1, 1, 0]
    wide = CC.triangle(t=0.3, margin=0.1)                            # t above every edge: tm2 is the rest distance itself
    (idx, tm2), counts, _ = cloth.contact_lists_reference(wide, wide.x0)
    CC.assert_lists_are_plain(wide, wide.x0, ((idx, tm2), counts, _), "wide triangle")
    assert counts.tolist() == [2, 2, 2] and tm2[0, 0] == CC.sq(wide.x0[0], wide.x0[1]) < wide.collision["t2"]


def test_lists_of_the_folded_strip_equal_a_plain_double_loop(folded):
    g, (x, _) = folded
    got = cloth.contact_lists_reference(g, x)
    CC.assert_lists_are_plain(g, x, got, "strip")
    CC.assert_lists_are_plain(g, x, cloth.contact_lists_reference(g, x, chunk=7), "strip in chunks of 7")
    assert got[1].max() > 30 and got[2].sum() == 0                   # folded: lists far longer than a flat sheet's, none cut


def test_a_pair_at_rest_distance_zero_is_out_and_the_cut_keeps_the_smallest():
    X, faces = with_coincident()
    g = cloth.garment(X, faces, 0, CC.params(t=0.15, margin=0.1))
    got = cloth.contact_lists_reference(g, g.x0)
    CC.assert_lists_are_plain(g, g.x0, got, "coincident")
    (idx, _), counts, _ = got
    assert 7 not in idx[6, :counts[6]] and 6 not in idx[7, :counts[7]] and counts[6] > 3
    cut = CC.with_constants(g, t=0.15, margin=0.1, K=6)
    (idx6, tm6), n6, over6 = cloth.contact_lists_reference(cut, g.x0)
    CC.assert_lists_are_plain(cut, g.x0, ((idx6, tm6), n6, over6), "K = 6")
    assert over6.sum() > 0 and (n6 + over6 == counts + got[2]).all()
    for i in range(len(X)):
        assert idx6[i, :n6[i]].tolist() == idx[i, :counts[i]][:6].tolist()


def test_the_bound_is_inclusive():
    # r = 0.75 + 0.25 = 1 and r2 = 1 exactly: a pair at distance 1 is in, one an ulp further is out
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, np.nextafter(1.0, 2.0), 0.0], [0.0, 0.0, -1.0]])
    g = CC.points(x + 0.0, t=0.75, margin=0.25)
    assert g.collision["r2"] == 1.0
    (idx, tm2), counts, _ = cloth.contact_lists_reference(g, x)
    assert idx[0, :counts[0]].tolist() == [1, 3] and counts.tolist() == [2, 1, 0, 1]
    assert tm2[0, 0] == 0.75 * 0.75


# ------------------------------------------------------------------------------------------------ invariants, no tolerance
def test_without_gravity_nothing_moves_and_the_grip_stays():
    g = cloth.garment(*sheet(41, 5, seed=3, size=0.8, jitter=0.1, flat=True), CC.STRIP_GRIP, CC.params(gravity=0.0))
    x, v, stats = cloth.simulate_reference(g, 20, stats=True)
    assert np.array_equal(x, g.x0) and not v.any()
    assert stats["contact_active"] == 0 and stats["contact_travel"] == 0.0 and stats["contact_max_list"] > 0


def test_the_grip_vertex_stays_at_the_origin(folded):
    g, (x, v) = folded
    assert not x[CC.STRIP_GRIP].any() and not v[CC.STRIP_GRIP].any() and np.abs(x).max() > 0.1


def test_thickness_zero_gives_the_bits_of_the_solver_without_contacts():
    off = CC.strip(t=0)
    assert off.collision is None and off.consts == CC.strip().consts
    x, v = cloth.state_arrays(off, None, None)
    for _ in range(150):                                             # the substep as it was: no lists, no pass
        cloth.substep(off, x, v)
    got = cloth.simulate_reference(off, 150, stats=True)
    assert np.array_equal(got[0], x) and np.array_equal(got[1], v) and got[2] == STATS0
    assert len(cloth.simulate_reference(off, 3)) == 2


def test_runs_split_at_multiples_of_the_rebuild_interval_are_one_run():
    g = CC.strip(R=5)                                                # 5 divides 50
    want = cloth.simulate_reference(g, 200, stats=True)
    x = v = None
    active = over = 0
    for _ in range(4):
        x, v, s = cloth.simulate_reference(g, 50, x, v, stats=True)
        active, over = active + s["contact_active"], over + s["contact_overflow"]
    assert np.array_equal(x, want[0]) and np.array_equal(v, want[1]) and active == want[2]["contact_active"] and over == want[2]["contact_overflow"]


# ------------------------------------------------------------------------------------------------ the scenario
def closest(x):
    d = x[CC.LEFT][:, None, :] - x[CC.RIGHT][None, :, :]
    return float(np.sqrt((d * d).sum(axis=-1)).min())


def fold(g, substeps):
    """-> (the smallest distance of a vertex of rows 0-15 to one of rows 25-40 over the substeps of the run, in cells, the diagnostics)"""
    near = [np.inf]

    def observe(s, x, v):
        near[0] = min(near[0], closest(x))
    stats = cloth.simulate_reference(g, substeps, stats=True, observe=observe)[2]
    return near[0] / CC.CELL, stats


def test_the_halves_of_the_folding_strip_stay_apart_with_contacts_and_pass_through_each_other_without():
    """1500 substeps of the strip.  With contacts the halves stay above 1.25 x the largest circumradius of a rest face (the hole a vertex could slip
    through, a quarter allowed for stretched faces), without them they come closer than a tenth of a cell.  Measured: 1.47 cells with contacts (overflow 0, travel 0.54, longest list 49), 0.028 cells without."""
    g = CC.strip()
    tri = g.x0[np.asarray(sheet(41, 5, seed=3, size=0.8, jitter=0.1, flat=True)[1])]
    a, b, c = (np.linalg.norm(tri[:, i] - tri[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0)))
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    hole = 1.25 * float((a * b * c / (4.0 * area)).max()) / CC.CELL
    on, stats = fold(g, 1500)
    off, _ = fold(CC.strip(t=0), 1500)
    print(f"closest approach of the halves: {on:.3f} cells with contacts, {off:.3f} without; bound {hole:.3f}; {stats}")
    assert 0.9 < hole < 1.1
    assert on > hole
    assert stats["contact_overflow"] == 0 and stats["contact_travel"] <= 1 and stats["contact_active"] > 0
    assert off < 0.1


# ------------------------------------------------------------------------------------------------ parameters
def test_parameter_refusals():
    for kw, msg in (({"margin": 0.0}, "collision_margin must be positive"), ({"R": 0}, "collision_rebuild"), ({"K": 0}, "collision_max_list"),
                    ({"K": 65}, "collision_max_list"), ({"relax": 0.0}, "collision_relax"), ({"relax": 1.5}, "collision_relax"),
                    ({"t": -0.01}, "must not be negative"), ({"t": float("nan")}, "finite")):
        with pytest.raises(ValueError, match=msg):
            CC.params(**kw)
    with pytest.raises(ValueError, match="contacts off"):
        cloth.contact_lists_reference(CC.strip(t=0), CC.strip().x0)
    c = cloth.collision_constants(CC.params(t=0.03, margin=0.01))
    assert c["t2"] == 0.03 * 0.03 and c["r"] == 0.03 + 0.01 and c["r2"] == c["r"] * c["r"] and c["half_margin"] == 0.005 and (c["K"], c["R"]) == (64, 2)
    assert cloth.collision_constants(CC.params(t=0)) is None


# ------------------------------------------------------------------------------------------------ simulate
FLAGS = ["--h", "0.004", "--duration", "0.4", "--damping", "2", "--alpha_stretch", "0", "--alpha_bend", "0.01", "--density", "0.25", "--gravity", "9.81"]


def test_simulate_with_self_collision_records_parameters_and_diagnostics(tmp_path, capsys):
    meshes = [open_box_mesh(0, n=3), open_box_mesh(1, n=4, drop=1)]
    plain, on, tight = (str(tmp_path / f"{n}.zarr") for n in ("plain", "on", "tight"))
    for path in (plain, on, tight):
        keys = write_canonical_store(path, meshes)
    SIM.main(["--zarr_in", plain, "--backend", "numpy"] + FLAGS)
    out = SIM.main(["--zarr_in", on, "--backend", "numpy", "--self_collision", "--collision_rebuild", "2"] + FLAGS)
    assert out["written"] == 2 and out["contact_warnings"] == []
    a, b = (zarr_store.open_group(p, create=False) for p in (plain, on))
    for key in keys:
        ra, rb = (r["samples"][key]["mesh"].attrs["cloth_simulation"] for r in (a, b))
        assert not any(k.startswith(("collision_", "contact_")) for k in ra)
        assert set(rb) - set(ra) == set(cloth.COLLISION_FIELDS) | set(cloth.CONTACT_STATS)
        mesh = b["samples"][key]["mesh"]
        g = cloth.garment_from_nocs(mesh["cloth_nocs_verts"][:], mesh["cloth_faces_tri"][:], rb["grip_vertex_idx"], rb["rest_scale"],
                                    cloth.ClothParams(gravity=9.81, h=0.004, damping=2.0, alpha_stretch=0.0, alpha_bend=0.01, density=0.25))
        assert rb["collision_thickness"] == cloth.DEFAULT_COLLISION_THICKNESS_FACTOR * cloth.mean_stretch_rest_length(g)
        assert rb["collision_margin"] == rb["collision_thickness"] and rb["collision_rebuild"] == 2 and rb["collision_max_list"] == 64
        assert rb["contact_overflow"] == 0 and rb["contact_max_list"] > 0 and 0 < rb["contact_travel"] <= 1
        on_params = cloth.ClothParams(gravity=9.81, h=0.004, damping=2.0, alpha_stretch=0.0, alpha_bend=0.01, density=0.25,
                                      **{k: rb[k] for k in cloth.COLLISION_FIELDS})
        want = cloth.simulate_reference(dataclasses.replace(g, collision=cloth.collision_constants(on_params)), 100, stats=True)
        assert np.array_equal(mesh["cloth_verts"][:], want[0].astype(np.float32)) and {k: rb[k] for k in cloth.CONTACT_STATS} == want[2]
    # a list of two entries and a margin of a hundredth of the thickness: cut lists and too much travel, named in a warning
    capsys.readouterr()
    out = SIM.main(["--zarr_in", tight, "--backend", "numpy", "--self_collision", "--collision_max_list", "2", "--collision_thickness", "0.2",
                    "--collision_margin", "0.002", "--collision_rebuild", "5"] + FLAGS)
    assert out["contact_warnings"] == keys
    rows = [json.loads(line) for line in capsys.readouterr().out.splitlines()]
    warnings = [r["warning"] for r in rows if "warning" in r]
    assert len(warnings) == 2 and all(k in w and "contact_overflow" in w for k, w in zip(keys, warnings))
    recs = [zarr_store.open_group(tight, create=False)["samples"][k]["mesh"].attrs["cloth_simulation"] for k in keys]
    print([(r["contact_overflow"], r["contact_travel"]) for r in recs])
    assert all(r["contact_overflow"] > 0 or r["contact_travel"] > 1 for r in recs) and any(r["contact_overflow"] > 0 for r in recs)


def test_simulate_without_the_flag_writes_the_store_it_always_wrote(tmp_path):
    path = str(tmp_path / "plain.zarr")
    keys = write_canonical_store(path, [open_box_mesh(0, n=3)])
    SIM.main(["--zarr_in", path, "--backend", "numpy"] + FLAGS)
    rec = zarr_store.open_group(path, create=False)["samples"][keys[0]]["mesh"].attrs["cloth_simulation"]
    assert set(rec) == {"gravity", "h", "damping", "alpha_stretch", "alpha_bend", "density", "duration", "substeps", "rest_scale", "grip_vertex_idx",
                        "kinetic_energy", "max_stretch_strain", "massless_vertices"}
