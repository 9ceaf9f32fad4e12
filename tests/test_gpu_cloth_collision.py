"""GPU (-m gpu): the self-collision of csrc/cloth.hip against the numpy restatement of garmentnets_amd/cloth.py, bit for bit (torch.equal, no tolerance):
the contact lists of gn_cloth_contact_lists (ops.cloth_contact_lists) against the brute-force lists, the solver with its contact pass
(ops.cloth_simulate_batch on garments with contacts on) against simulate_reference on both storage paths, at several workgroup sizes, rebuild intervals
and launch chunkings, the diagnostics, the refusals, and `simulate --self_collision` end to end.  tests/test_cloth_collision_host.py holds the
restatement itself to the definition."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cloth_collision_cases as CC  # noqa: E402
from cloth_cases import sheet, write_canonical_store  # noqa: E402
from garmentnets_amd import _lib, cloth, ops  # noqa: E402
from garmentnets_amd import prepare as P  # noqa: E402
from garmentnets_amd import simulate as SIM  # noqa: E402
from garmentnets_amd.io import zarr_store  # noqa: E402
from test_winding_host import open_box_mesh  # noqa: E402

DEV = "cuda:0"
WARM, STEPS = 384, 64


@pytest.fixture(scope="module")
def folded():
    """the strip, its state after WARM substeps of the restatement (the halves have met), and the restatement of STEPS more per variant, computed once
    and left unchanged: name -> (garment, (x, v, stats))"""
    g = CC.strip()
    start = cloth.simulate_reference(g, WARM)
    variants = {"R2": g, "R1": CC.with_constants(g, R=1), "R5": CC.with_constants(g, R=5), "K6": CC.with_constants(g, K=6),
                "relax": CC.with_constants(g, relax=0.5)}
    return start, {n: (v, cloth.simulate_reference(v, STEPS, *start, stats=True)) for n, v in variants.items()}


def same_state(got, want, tag):
    (x, v), stats = got
    assert x.dtype == v.dtype == torch.float64
    assert torch.equal(x.cpu(), torch.from_numpy(want[0])), (tag, "x", (x.cpu() - torch.from_numpy(want[0])).abs().max().item())
    assert torch.equal(v.cpu(), torch.from_numpy(want[1])), (tag, "v", (v.cpu() - torch.from_numpy(want[1])).abs().max().item())
    assert stats == want[2], (tag, stats, want[2])


def run(g, start, **kw):
    states, stats = ops.cloth_simulate_batch([g], STEPS, states=[start], stats=True, device=DEV, **kw)
    return states[0], stats[0]


# ------------------------------------------------------------------------------------------------ lists
def lists_numpy(got):
    (idx, tm2), counts, overflow = got
    return (idx.cpu().numpy(), tm2.cpu().numpy()), counts.cpu().numpy(), overflow.cpu().numpy()


def assert_device_lists(g, x, tag):
    want = cloth.contact_lists_reference(g, x)
    got = lists_numpy(ops.cloth_contact_lists([g], [(x, None)], device=DEV)[0])
    assert np.array_equal(got[0][0], want[0][0]), (tag, "indices")
    assert np.array_equal(got[0][1], want[0][1]), (tag, "tm2")
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (tag, "counts")
    return want


def test_lists_of_one_vertex_and_of_a_triangle():
    one = CC.points(np.zeros((1, 3)))
    (idx, _), counts, overflow = assert_device_lists(one, one.x0, "one vertex")
    assert counts.tolist() == [0] and overflow.tolist() == [0] and (idx == -1).all()
    tri = CC.triangle(t=0.15, margin=0.08)
    assert assert_device_lists(tri, tri.x0, "triangle")[1].tolist() == [1, 1, 0]
    CC.assert_lists_are_plain(tri, tri.x0, lists_numpy(ops.cloth_contact_lists([tri], device=DEV)[0]), "triangle against the plain loop")


def test_lists_of_the_folded_strip(folded):
    (x, _), variants = folded
    assert assert_device_lists(variants["R2"][0], x, "strip")[1].max() > 30
    cut = assert_device_lists(variants["K6"][0], x, "strip, K = 6")
    assert cut[1].max() == 6 and cut[2].sum() > 1000


def test_lists_of_a_sheet_whose_size_is_no_multiple_of_the_wave():
    X, faces = sheet(9, 7, seed=12)
    g = cloth.garment(X, faces, 30, CC.params(t=0.06, margin=0.05))
    assert len(g.w) == 63
    assert assert_device_lists(g, g.x0, "9x7")[1].min() > 3
    bent = cloth.simulate_reference(g, 40)[0]
    assert_device_lists(g, bent, "9x7 after 40 substeps")


def test_lists_of_seventy_vertices_in_one_cell():
    g = CC.packed(70)
    (idx, _), counts, overflow = assert_device_lists(g, g.x0, "packed")
    assert (counts == 64).all() and overflow.tolist() == [5 if i not in (4, 5) else 4 for i in range(70)]
    assert 5 not in idx[4] and 4 not in idx[5]                       # coincident at rest: excluded
    assert_device_lists(CC.packed(70, K=6), g.x0, "packed, K = 6")


def test_lists_of_three_hundred_vertices_within_reach_of_each_other():
    # more partners than the query kernel holds in LDS (256): it draws the K smallest one after the other
    for K in (64, 6):
        g = CC.packed(300, K=K)
        _, counts, overflow = assert_device_lists(g, g.x0, f"300 packed, K = {K}")
        assert (counts == K).all() and overflow.min() == 298 - K and overflow.max() == 299 - K


def test_lists_on_cell_borders_at_negative_coordinates_and_exactly_at_r():
    g, x = CC.on_borders(t=0.02, margin=0.01)
    want = assert_device_lists(g, x, "borders")
    assert want[1].max() > 2 and (x < 0).any()
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, np.nextafter(1.0, 2.0), 0.0], [0.0, 0.0, -1.0]])
    at_r = CC.points(x + 0.0, t=0.75, margin=0.25)
    assert at_r.collision["r2"] == 1.0
    assert assert_device_lists(at_r, x, "a pair exactly at r")[1].tolist() == [2, 1, 0, 1]


def test_lists_of_a_ragged_batch_equal_each_garment_alone(folded):
    (x, _), variants = folded
    kw = dict(t=1.5 * CC.CELL)
    gs = [variants["R2"][0], CC.triangle(**kw), CC.packed(70, **kw)]
    states = [(x, None), None, None]
    got = ops.cloth_contact_lists(gs, states, device=DEV)
    for g, s, batch in zip(gs, states, got):
        alone = ops.cloth_contact_lists([g], [s], device=DEV)[0]
        want = cloth.contact_lists_reference(g, g.x0 if s is None else s[0])
        for a, b, c in zip(lists_numpy(batch), lists_numpy(alone), want):
            if isinstance(c, tuple):
                assert all(np.array_equal(p, r) and np.array_equal(q, r) for p, q, r in zip(a, b, c))
            else:
                assert np.array_equal(a, c) and np.array_equal(b, c)
    back = ops.cloth_contact_lists(gs, states, backend="numpy")[2]
    assert torch.equal(back[0][0], got[2][0][0].cpu()) and torch.equal(back[1], got[2][1].cpu())


# ------------------------------------------------------------------------------------------------ the solver
def test_the_restatement_has_contacts_in_the_compared_substeps(folded):
    start, variants = folded
    g, (x, v, stats) = variants["R2"]
    assert stats["contact_active"] > 5000 and stats["contact_overflow"] == 0 and 0 < stats["contact_travel"] <= 1 and stats["contact_max_list"] > 30
    assert np.isfinite(x).all() and np.abs(x - start[0]).max() > 1e-3
    k6 = variants["K6"][1][2]
    assert k6["contact_overflow"] > 1000 and k6["contact_active"] > 0 and np.isfinite(variants["K6"][1][0]).all()
    lists, counts, _ = cloth.contact_lists_reference(g, start[0])
    live = g.w > 0
    assert any(CC.STRIP_GRIP in lists[0][i, :counts[i]] for i in np.flatnonzero(live)), "no list holds the held vertex"


@pytest.mark.parametrize("name", ["R2", "R1", "R5", "K6", "relax"])
def test_device_equals_the_restatement(folded, name):
    start, variants = folded
    g, want = variants[name]
    same_state(run(g, start), want, name)
    same_state(run(g, start, block=64), want, name + ", block 64")


def test_both_storage_paths_and_every_workgroup_size(folded):
    start, variants = folded
    g, want = variants["R2"]
    need = 24 * len(g.w)
    assert ops.cloth_storage_path(g, need) == "lds" and ops.cloth_storage_path(g, need - 1) == "global"
    for kw in ({"lds_budget": need}, {"lds_budget": need - 1}, {"lds_budget": 0}):
        for block in (64, 192, 1024):
            same_state(run(g, start, block=block, **kw), want, f"{kw}, block {block}")


@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_launch_chunking_changes_no_bit(folded, chunk):
    start, variants = folded
    for name in ("R2", "R5"):
        g, want = variants[name]
        same_state(run(g, start, max_substeps_per_launch=chunk), want, f"{name}, launches of {chunk}")
    same_state(run(variants["R5"][0], start, max_substeps_per_launch=chunk, lds_budget=0), variants["R5"][1], f"R5, launches of {chunk}, global")


def test_a_batch_with_a_triangle_and_the_output_without_stats(folded):
    start, variants = folded
    g, want = variants["R2"]
    tri = CC.triangle()
    tri_want = cloth.simulate_reference(tri, STEPS, stats=True)
    assert tri_want[2]["contact_active"] == 0 and tri_want[2]["contact_max_list"] == 0
    states, stats = ops.cloth_simulate_batch([tri, g, tri], STEPS, states=[None, start, None], stats=True, device=DEV, block=128)
    same_state((states[1], stats[1]), want, "the strip between two triangles")
    same_state((states[0], stats[0]), tri_want, "triangle")
    same_state((states[2], stats[2]), tri_want, "triangle at offset 2")
    plain = ops.cloth_simulate_batch([g], STEPS, states=[start], device=DEV)
    assert isinstance(plain, list) and len(plain[0]) == 2 and torch.equal(plain[0][0].cpu(), torch.from_numpy(want[0]))
    got = ops.cloth_simulate_batch([g], STEPS, states=[start], stats=True, backend="numpy")
    same_state((got[0][0], got[1][0]), want, "numpy backend")
    zero = ops.cloth_simulate_batch([g], 0, states=[start], stats=True, device=DEV)
    assert torch.equal(zero[0][0][0].cpu(), torch.from_numpy(start[0])) and zero[1][0] == {"contact_overflow": 0, "contact_max_list": 0,
                                                                                          "contact_travel": 0.0, "contact_active": 0}


def test_contacts_off_route_to_the_entry_without_them():
    off = CC.strip(t=0)
    want = cloth.simulate_reference(off, 100, stats=True)
    states, stats = ops.cloth_simulate_batch([off], 100, stats=True, device=DEV)
    same_state((states[0], stats[0]), want, "contacts off")
    with pytest.raises(ValueError, match="contacts off"):
        ops.cloth_contact_lists([off], device=DEV)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(folded):
    start, variants = folded
    g = variants["R2"][0]
    with pytest.raises(ValueError, match="share their collision constants"):
        ops.cloth_simulate_batch([g, variants["R5"][0]], 4, device=DEV)
    with pytest.raises(ValueError, match="share their collision constants"):
        ops.cloth_contact_lists([g, CC.strip(t=0)], device=DEV)
    for change, msg in (({"K": 65}, "K=65 outside"), ({"K": 0}, "K=0 outside"), ({"R": 0}, "R=0 < 1"), ({"r2": float("inf")}, "r2=inf is not finite"),
                        ({"t2": float("nan")}, "t2=nan is not finite"), ({"relax": 2.0}, "collision_relax=2.0 outside")):
        broken = dataclasses.replace(g, collision=dict(g.collision, **change))
        with pytest.raises(ValueError, match=msg):
            ops.cloth_simulate_batch([broken], 4, device=DEV)
        with pytest.raises(ValueError, match=msg):
            ops.cloth_contact_lists([broken], device=DEV)
    # the entries' own limits, by name and before any launch
    dev = torch.device(DEV)
    t = ops.cloth_device_tables([g], [start], dev)
    col = ops.cloth_collision_constants([g], "test")
    c = ops.cloth_contact_buffers([g], t, col, dev)
    flag = torch.zeros(1, dtype=torch.int64, device=DEV)

    def lists(K=64, flags=2, buckets=None, consts=None, ws=None, max_verts=None, nv=None):
        h = col["host"] if consts is None else (ctypes.c_double * 4)(*consts)
        _lib.call("gn_cloth_contact_lists", ops._p(t["x"]), ops._p(c["x0"]), ops._p(t["csr"]), 1, t["total_verts"] if nv is None else nv,
                  c["max_verts"] if max_verts is None else max_verts, c["buckets"] if buckets is None else buckets, ctypes.cast(h, ctypes.c_void_p), K,
                  flags, ops._p(c["workspace"]), c["workspace_bytes"] if ws is None else ws, ops._p(c["list_j"]), ops._p(c["list_tm2"]),
                  ops._p(c["list_n"]), ops._p(c["list_total"]), ops._p(c["diag"]), ops._stream())

    def solver(K=64, consts=None, block=64, substeps=2):
        h = col["host"] if consts is None else (ctypes.c_double * 4)(*consts)
        _lib.call("gn_cloth_simulate_contacts_batch", ops._p(t["x"]), ops._p(t["v"]), ops._p(t["w"]), ops._p(t["pairs"]), ops._p(t["l0"]),
                  ops._p(t["alpha_t"]), ops._p(t["csr"]), ops._p(t["colour_off"]), 1, t["total_verts"], t["total_constraints"], substeps, 50,
                  ctypes.cast(t["consts"], ctypes.c_void_p), 0, block, ops._p(flag), ops._p(c["list_j"]), ops._p(c["list_tm2"]), ops._p(c["list_n"]), K,
                  ctypes.cast(h, ctypes.c_void_p), ops._p(c["corr"]), ops._p(c["diag"]), ops._stream())
    t2, r2, cell, relax = list(col["host"])
    before = t["x"].clone()
    for kw, msg in (({"K": 0}, "K=0 outside"), ({"K": 65}, "K=65 outside"), ({"flags": 0}, "flags=0"), ({"flags": 4}, "flags=4"),
                    ({"buckets": 96}, "buckets=96"), ({"buckets": 64}, "buckets=64"), ({"consts": [t2, float("nan"), cell, relax]}, "constant 1 is not finite"),
                    ({"consts": [0.0, r2, cell, relax]}, "constant 0 is not finite and positive"), ({"consts": [t2, r2, col["r"], relax]}, "does not exceed r"),
                    ({"ws": c["workspace_bytes"] - 1}, "workspace of"), ({"max_verts": 206}, "max_verts=206"), ({"nv": 2 ** 31 // 64}, "below 2\\^31")):
        with pytest.raises(ValueError, match=msg):
            lists(**kw)
    for kw, msg in (({"K": 0}, "K=0 outside"), ({"K": 65}, "K=65 outside"), ({"consts": [t2, r2, cell, float("nan")]}, "relax"),
                    ({"consts": [t2, r2, cell, 0.0]}, "relax"), ({"block": 96}, "block=96"), ({"substeps": -1}, "substeps=-1")):
        with pytest.raises(ValueError, match=msg):
            solver(**kw)
    torch.cuda.synchronize()
    assert torch.equal(t["x"], before) and flag.item() == 0 and not c["diag"].any() and not c["list_n"].any()
    assert ops.cloth_contact_lists([], device=DEV) == [] and ops.cloth_simulate_batch([], 5, stats=True, device=DEV) == []


def test_a_corrupted_list_index_is_flagged_and_never_dereferenced(folded):
    start, variants = folded
    g, want = variants["R2"]
    tri = CC.triangle()
    gs = [tri, g]
    dev = torch.device(DEV)
    col = ops.cloth_collision_constants(gs, "test")
    for lds in (24 * len(g.w), 0):
        t = ops.cloth_device_tables(gs, [cloth.state_arrays(tri, None, None), start], dev)
        c = ops.cloth_contact_buffers(gs, t, col, dev)
        n, pad = t["total_verts"], 8
        bufs = {}
        for k, src in (("x", t["x"]), ("v", t["v"]), ("corr", c["corr"])):
            bufs[k] = torch.full((n + 2 * pad, 3), 7.25, dtype=torch.float64, device=DEV)
            bufs[k][pad:pad + n] = src
        t["x"] = bufs["x"][pad:pad + n]
        ops._cloth_lists_call(t, c, col, 2, _lib.CLOTH_LISTS_BUILD)
        row = 3 + 40                                                 # a vertex of the strip whose list is not empty
        assert c["list_n"][row].item() > 2
        c["list_j"][row, 0] = len(g.w)                               # one past the last vertex
        c["list_j"][row, 2] = -1
        flag = torch.zeros(1, dtype=torch.int64, device=DEV)
        _lib.call("gn_cloth_simulate_contacts_batch", ops._p(bufs["x"][pad:]), ops._p(bufs["v"][pad:]), ops._p(t["w"]), ops._p(t["pairs"]), ops._p(t["l0"]),
                  ops._p(t["alpha_t"]), ops._p(t["csr"]), ops._p(t["colour_off"]), 2, n, t["total_constraints"], 2, 50,
                  ctypes.cast(t["consts"], ctypes.c_void_p), lds, 64, ops._p(flag), ops._p(c["list_j"]), ops._p(c["list_tm2"]), ops._p(c["list_n"]),
                  col["K"], ctypes.cast(col["host"], ctypes.c_void_p), ops._p(bufs["corr"][pad:]), ops._p(c["diag"]), ops._stream())
        assert flag.item() == 1
        with pytest.raises(IndexError):
            ops._raise_bad_face(flag.item(), "cloth_simulate")
        for k in bufs:
            assert bool((bufs[k][:pad] == 7.25).all()) and bool((bufs[k][pad + n:] == 7.25).all()), (k, lds)
        assert bool(bufs["x"][pad:pad + n].isfinite().all())
        tri_want = cloth.simulate_reference(tri, 2)
        assert torch.equal(bufs["x"][pad:pad + 3].cpu(), torch.from_numpy(tri_want[0])), "the good garment of the same launch"


# ------------------------------------------------------------------------------------------------ simulate, end to end
def test_simulate_with_self_collision_on_the_device_equals_the_numpy_backend_and_feeds_prepare(tmp_path):
    meshes = [open_box_mesh(0, n=3), open_box_mesh(1, n=4, drop=1)]
    flags = ["--h", "0.004", "--duration", "0.4", "--damping", "2", "--alpha_stretch", "0", "--alpha_bend", "0.01", "--density", "0.25", "--gravity", "9.81",
             "--self_collision", "--collision_rebuild", "3"]
    stores = {}
    for backend in ("hip", "numpy"):
        stores[backend] = str(tmp_path / f"{backend}.zarr")
        keys = write_canonical_store(stores[backend], meshes)
        out = SIM.main(["--zarr_in", stores[backend], "--backend", backend, "--batch_size", "2"] + flags)
        assert out["written"] == 2 and out["substeps"] == 100 and out["summary_written"] and out["contact_warnings"] == []
    a, b = (zarr_store.open_group(stores[k], create=False) for k in ("hip", "numpy"))
    for key in keys:
        x, y = a["samples"][key]["mesh"]["cloth_verts"][:], b["samples"][key]["mesh"]["cloth_verts"][:]
        assert x.dtype == np.float32 and np.array_equal(x, y) and np.abs(x).max() > 0.1
        ra, rb = (r["samples"][key]["mesh"].attrs["cloth_simulation"] for r in (a, b))
        assert ra == rb and ra["collision_rebuild"] == 3 and ra["contact_max_list"] > 0
    assert np.array_equal(a["summary"]["cloth_aabb_union"][:], b["summary"]["cloth_aabb_union"][:])
    done = P.main(["--zarr_in", stores["hip"], "--volume_size", "24", "--point_clouds", "--pc_img_size", "96"])
    assert done["written"]["point_cloud"] == 2 and done["written"]["sim_nocs_winding_number_field"] == 2
