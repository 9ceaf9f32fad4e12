"""GPU (-m gpu): the vertex-face contacts of csrc/cloth.hip against the numpy restatement of garmentnets_amd/cloth.py, bit for bit (torch.equal /
array_equal, no tolerance): the face-contact lists of gn_cloth_face_contact_lists (ops.cloth_face_contact_lists) against the brute-force lists, the
solver with face entries (gn_cloth_simulate_face_contacts_batch through ops.cloth_simulate_batch) against simulate_reference on both storage paths,
at several workgroup sizes, rebuild intervals and launch chunkings, the seven diagnostics, the refusals, a bad face index, and
`simulate --self_collision --face_contacts` end to end.  tests/test_cloth_face_host.py holds the restatement itself to the definition."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cloth_collision_cases as CC  # noqa: E402
import cloth_face_cases as FC  # noqa: E402
from cloth_cases import write_canonical_store  # noqa: E402
from garmentnets_amd import _lib, cloth, ops  # noqa: E402
from garmentnets_amd import simulate as SIM  # noqa: E402
from garmentnets_amd.io import zarr_store  # noqa: E402
from test_winding_host import open_box_mesh  # noqa: E402

DEV = "cuda:0"
BEFORE, STEPS = 88, 64                     # the dart reaches the shell of the face at substep 96
SEVEN = cloth.CONTACT_STATS + cloth.FACE_CONTACT_STATS


@pytest.fixture(scope="module")
def darts():
    """the dart's state BEFORE substeps into its fall and the restatement of STEPS more per variant, computed once and left unchanged:
    (start, name -> (garment, (x, v, stats)))"""
    g, v0 = FC.dart()
    start = cloth.simulate_reference(g, BEFORE, g.x0, v0)
    variants = {"R2": g, "R1": FC.dart(R=1)[0], "R5": FC.dart(R=5)[0], "relax": FC.dart(relax=0.5)[0]}
    return start, {n: (v, cloth.simulate_reference(v, STEPS, *start, stats=True)) for n, v in variants.items()}


@pytest.fixture(scope="module")
def folded():
    """the folding strip after 384 substeps with vertex contacts only (the halves have met), then 16 substeps of the restatement with face contacts of
    three quarters of a cell on -> (garment, start, (x, v, stats), the stats of the first of those substeps alone)"""
    start = cloth.simulate_reference(CC.strip(), 384)
    g = FC.strip(tf=0.75 * CC.CELL)
    return g, start, cloth.simulate_reference(g, 16, *start, stats=True), cloth.simulate_reference(g, 1, *start, stats=True)[2]


def same_state(got, want, tag):
    (x, v), stats = got
    assert x.dtype == v.dtype == torch.float64
    assert torch.equal(x.cpu(), torch.from_numpy(want[0])), (tag, "x", (x.cpu() - torch.from_numpy(want[0])).abs().max().item())
    assert torch.equal(v.cpu(), torch.from_numpy(want[1])), (tag, "v", (v.cpu() - torch.from_numpy(want[1])).abs().max().item())
    assert stats == want[2] and tuple(stats) == SEVEN, (tag, stats, want[2])


def run(g, start, steps=STEPS, **kw):
    states, stats = ops.cloth_simulate_batch([g], steps, states=[start], stats=True, device=DEV, **kw)
    return states[0], stats[0]


# ------------------------------------------------------------------------------------------------ lists
def lists_numpy(got):
    (idx, tm2), counts, overflow = got
    return (idx.cpu().numpy(), tm2.cpu().numpy()), counts.cpu().numpy(), overflow.cpu().numpy()


def assert_same_lists(got, want, tag):
    assert got[0][0].dtype == np.int32 and got[0][1].dtype == np.float64 and got[0][0].shape == want[0][0].shape, tag
    assert np.array_equal(got[0][0], want[0][0]), (tag, "indices and the fill of the rows")
    assert np.array_equal(got[0][1], want[0][1]), (tag, "tm2")
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (tag, "counts, overflow")


def assert_device_lists(g, x, tag, **kw):
    want = cloth.face_contact_lists_reference(g, x)
    assert_same_lists(lists_numpy(ops.cloth_face_contact_lists([g], [(x, None)], device=DEV, **kw)[0]), want, tag)
    return want


@pytest.mark.parametrize("name", ["at_rf", "own_corner", "coincident_at_rest", "stacked_K3", "stacked"])
def test_lists_of_the_host_cases(name):
    g, x = FC.list_cases()[name]
    want = assert_device_lists(g, x, name)
    assert want[1].sum() > 0
    FC.assert_face_lists_are_plain(g, x, lists_numpy(ops.cloth_face_contact_lists([g], [(x, None)], device=DEV)[0]), name + " against the plain loop")
    assert_device_lists(g, x, name + ", more face chunks than faces", chunks=7)


def test_lists_of_one_face_and_of_a_hundred_and_thirty():
    g, x = FC.at_rf()                                                # 1 face
    assert len(g.faces) == 1 and assert_device_lists(g, x, "one face")[1].tolist() == [0, 0, 0, 1, 0, 1, 1]
    g, x = FC.bent_sheet()                                           # 84 vertices (no multiple of 64), 130 faces: one past a face tile
    assert len(g.w) == 84 and len(g.faces) == 130
    (idx, _), counts, overflow = assert_device_lists(g, x, "130 faces", chunks=1)
    assert idx.max() == 129 and counts.min() > 3 and overflow.sum() > 0 and counts.max() == 32
    for chunks in (2, 3, 64, 131, 1024):                             # the lists do not depend on the chunks; 131 and 1024: more chunks than faces
        assert_device_lists(g, x, f"130 faces in {chunks} chunks", chunks=chunks)
    cut, _ = FC.bent_sheet(Kf=3)
    (idx, _), counts, overflow = assert_device_lists(cut, x, "130 faces, Kf = 3")
    assert counts.max() == 3 and overflow.sum() > 500
    assert_device_lists(cut, x, "130 faces, Kf = 3, 5 chunks", chunks=5)


def test_lists_of_a_ragged_batch_equal_each_garment_alone():
    sheet, x = FC.bent_sheet()
    kw = dict(t=0.06, margin=0.05, tf=0.04)
    gs = [FC.with_constants(FC.stacked(32)[0], **kw), sheet, FC.with_constants(FC.own_corner()[0], **kw)]
    states = [None, (x, None), None]
    for chunks in (None, 4):
        got = ops.cloth_face_contact_lists(gs, states, device=DEV, chunks=chunks)
        for g, s, batch in zip(gs, states, got):
            alone = ops.cloth_face_contact_lists([g], [s], device=DEV, chunks=chunks)[0]
            want = cloth.face_contact_lists_reference(g, g.x0 if s is None else s[0])
            assert_same_lists(lists_numpy(batch), want, f"in the batch, chunks {chunks}")
            assert_same_lists(lists_numpy(alone), want, f"alone, chunks {chunks}")
    back = ops.cloth_face_contact_lists(gs, states, backend="numpy")[1]
    assert torch.equal(back[0][0], got[1][0][0].cpu()) and torch.equal(back[1], got[1][1].cpu())


# ------------------------------------------------------------------------------------------------ the solver
def test_the_restatement_stops_the_dart_in_the_compared_substeps(darts):
    start, variants = darts
    assert start[0][3:, 2].min() > 1.3 * FC.T_F, "the start state lies before the contact"
    for name, (g, (x, v, stats)) in variants.items():
        assert stats["face_contact_active"] > 0 and stats["face_contact_overflow"] == 0 and stats["contact_travel"] <= 1, (name, stats)
        assert x[3:, 2].min() > 0.9 * FC.T_F and np.abs(v[3:, 2]).max() < 0.25, name
    assert variants["relax"][1][2]["face_contact_active"] > variants["R2"][1][2]["face_contact_active"]


@pytest.mark.parametrize("name", ["R2", "R1", "R5", "relax"])
def test_device_equals_the_restatement(darts, name):
    start, variants = darts
    g, want = variants[name]
    same_state(run(g, start), want, name)
    same_state(run(g, start, block=1024), want, name + ", block 1024")


def test_both_storage_paths_and_every_workgroup_size(darts):
    start, variants = darts
    g, want = variants["R2"]
    need = 24 * len(g.w)
    assert ops.cloth_storage_path(g, need) == "lds" and ops.cloth_storage_path(g, need - 1) == "global"
    for kw in ({"lds_budget": need}, {"lds_budget": need - 1}, {"lds_budget": 0}):
        for block in (64, 192, 1024):
            same_state(run(g, start, block=block, **kw), want, f"{kw}, block {block}")


@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_launch_chunking_changes_no_bit(darts, chunk):
    start, variants = darts
    for name in ("R2", "R5"):
        g, want = variants[name]
        same_state(run(g, start, max_substeps_per_launch=chunk), want, f"{name}, launches of {chunk}")
    same_state(run(variants["R5"][0], start, max_substeps_per_launch=chunk, lds_budget=0), variants["R5"][1], f"R5, launches of {chunk}, global")


def test_vertex_and_face_entries_active_in_the_same_substep(folded):
    g, start, want, first = folded
    assert first["contact_active"] > 0 and first["face_contact_active"] > 0, ("the case needs both kinds active in one substep", first)
    assert want[2]["contact_active"] > 100 and want[2]["face_contact_active"] > 100 and np.isfinite(want[0]).all()
    same_state(run(g, start, steps=16), want, "strip")
    same_state(run(g, start, steps=16, lds_budget=0, block=64), want, "strip, global, block 64")
    # in a ragged batch with the dart's garment rebuilt on the strip's constants
    p = FC.params(tf=0.75 * CC.CELL)
    small = cloth.garment(FC.DART_X, FC.DART_FACES, 0, p)
    small_want = cloth.simulate_reference(small, 16, stats=True)
    states, stats = ops.cloth_simulate_batch([small, g, small], 16, states=[None, start, None], stats=True, device=DEV, block=128)
    same_state((states[1], stats[1]), want, "the strip between two small garments")
    same_state((states[0], stats[0]), small_want, "small garment")
    same_state((states[2], stats[2]), small_want, "small garment at offset 2")
    got = ops.cloth_simulate_batch([g], 16, states=[start], stats=True, backend="numpy")
    same_state((got[0][0], got[1][0]), want, "numpy backend")


def test_face_thickness_zero_routes_to_the_entry_without_face_entries(darts, monkeypatch):
    start, _ = darts
    off = FC.dart(tf=0.0)[0]
    assert off.face_collision is None
    want = cloth.simulate_reference(off, STEPS, *start, stats=True)
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    states, stats = ops.cloth_simulate_batch([off], STEPS, states=[start], stats=True, device=DEV)
    assert set(called) == {"gn_cloth_contact_lists", "gn_cloth_simulate_contacts_batch"}
    assert torch.equal(states[0][0].cpu(), torch.from_numpy(want[0])) and torch.equal(states[0][1].cpu(), torch.from_numpy(want[1]))
    assert stats[0] == want[2] and tuple(stats[0]) == cloth.CONTACT_STATS and want[0][3:, 2].max() < 0
    with pytest.raises(ValueError, match="face contacts off"):
        ops.cloth_face_contact_lists([off], device=DEV)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(darts):
    start, variants = darts
    g = variants["R2"][0]
    for fn in (lambda gs: ops.cloth_simulate_batch(gs, 4, device=DEV), lambda gs: ops.cloth_face_contact_lists(gs, device=DEV)):
        with pytest.raises(ValueError, match="share their face-contact constants"):
            fn([g, FC.dart(tf=0.02)[0]])
        with pytest.raises(ValueError, match="share their face-contact constants"):
            fn([g, FC.dart(tf=0.0)[0]])
        with pytest.raises(ValueError, match="vertex contacts are off"):
            fn([dataclasses.replace(g, collision=None)])
        for change, msg in (({"Kf": 33}, "Kf=33 outside"), ({"Kf": 0}, "Kf=0 outside"), ({"rf2": float("inf")}, "rf2=inf is not finite"),
                            ({"tf2": float("nan")}, "tf2=nan is not finite"), ({"tf2": 0.0}, "tf2=0.0 is not finite and positive")):
            with pytest.raises(ValueError, match=msg):
                fn([dataclasses.replace(g, face_collision=dict(g.face_collision, **change))])
    with pytest.raises(ValueError, match="chunks=0 outside"):
        ops.cloth_face_contact_lists([g], device=DEV, chunks=0)
    with pytest.raises(ValueError, match="chunks=1025 outside"):
        ops.cloth_face_contact_lists([g], device=DEV, chunks=1025)
    # the entries' own limits, by name and before any launch
    dev = torch.device(DEV)
    t = ops.cloth_device_tables([g], [start], dev)
    col, fcol = ops.cloth_collision_constants([g], "test"), ops.cloth_face_collision_constants([g], "test")
    c = ops.cloth_contact_buffers([g], t, col, dev)
    fc = ops.cloth_face_buffers([g], t, fcol, dev, chunks=2)
    flag = torch.zeros(1, dtype=torch.int64, device=DEV)
    null = None

    def lists(Kf=32, chunks=2, consts=None, colh=col["host"], hit_entries=None, hit_rows=None, list_entries=None, list_rows=None, fdiag_rows=1,
              x=t["x"], B=1, list_f=fc["list_f"], nf=fc["total_faces"]):
        h = fcol["host"] if consts is None else (ctypes.c_double * 2)(*consts)
        _lib.call("gn_cloth_face_contact_lists", ops._p(x) if x is not None else null, ops._p(fc["x0"]), ops._p(t["csr"]), ops._p(fc["faces"]),
                  ops._p(fc["fcsr"]), B, t["total_verts"], nf, fc["max_verts"], ctypes.cast(h, ctypes.c_void_p),
                  ctypes.cast(colh, ctypes.c_void_p) if colh is not None else null, Kf, chunks, ops._p(fc["hit_f"]), ops._p(fc["hit_tm2"]),
                  fc["hit_f"].numel() if hit_entries is None else hit_entries, ops._p(fc["hit_n"]), fc["hit_n"].numel() if hit_rows is None else hit_rows,
                  ops._p(list_f) if list_f is not None else null, ops._p(fc["list_tm2"]),
                  fc["list_f"].numel() if list_entries is None else list_entries, ops._p(fc["list_n"]),
                  ops._p(fc["list_total"]), fc["list_n"].numel() if list_rows is None else list_rows, ops._p(fc["fdiag"]), fdiag_rows, ops._p(flag),
                  ops._stream())

    def solver(Kf=32, consts=None, colh=col["host"], flist_entries=None, flist_rows=None, fdiag_rows=1, faces=fc["faces"], block=64, substeps=2, K=64,
               flist_f=fc["list_f"], fdiag=fc["fdiag"], nf=fc["total_faces"]):
        h = fcol["host"] if consts is None else (ctypes.c_double * 2)(*consts)
        _lib.call("gn_cloth_simulate_face_contacts_batch", ops._p(t["x"]), ops._p(t["v"]), ops._p(t["w"]), ops._p(t["pairs"]), ops._p(t["l0"]),
                  ops._p(t["alpha_t"]), ops._p(t["csr"]), ops._p(t["colour_off"]), 1, t["total_verts"], t["total_constraints"], substeps, 50,
                  ctypes.cast(t["consts"], ctypes.c_void_p), 0, block, ops._p(flag), ops._p(c["list_j"]), ops._p(c["list_tm2"]), ops._p(c["list_n"]), K,
                  ctypes.cast(colh, ctypes.c_void_p) if colh is not None else null, ops._p(c["corr"]), ops._p(c["diag"]),
                  ops._p(faces) if faces is not None else null, ops._p(fc["fcsr"]), nf,
                  ops._p(flist_f) if flist_f is not None else null, ops._p(fc["list_tm2"]), fc["list_f"].numel() if flist_entries is None else flist_entries, ops._p(fc["list_n"]),
                  fc["list_n"].numel() if flist_rows is None else flist_rows, Kf, ctypes.cast(h, ctypes.c_void_p),
                  ops._p(fdiag) if fdiag is not None else null, fdiag_rows, ops._stream())
    tf2, rf2 = list(fcol["host"])
    before = t["x"].clone()
    n = t["total_verts"]
    for kw, msg in (({"Kf": 0}, "Kf=0 outside"), ({"Kf": 33}, "Kf=33 outside"), ({"chunks": 0}, "chunks=0 outside"), ({"chunks": 1025}, "chunks=1025"),
                    ({"consts": [tf2, float("nan")]}, "face constant 1 is not finite"), ({"consts": [0.0, rf2]}, "face constant 0 is not finite and positive"),
                    ({"consts": [float("inf"), rf2]}, "face constant 0"), ({"colh": None}, "null collision constants"),
                    ({"hit_entries": n * 2 * 32 - 1}, "hit buffers of"), ({"hit_rows": n * 2 - 1}, "hit buffers of"), ({"chunks": 3}, "hit buffers of"),
                    ({"list_entries": n * 32 - 1}, "lists of"), ({"list_rows": n - 1}, "lists of"), ({"fdiag_rows": 0}, "fdiag of 0 rows"),
                    ({"x": None}, "null pointer"), ({"B": 65536}, "B=65536"), ({"list_f": None}, "null list"),
                    ({"nf": (2 ** 31 - 1) // 3}, "faces: the tables must stay below 2\\^31")):
        with pytest.raises(ValueError, match=msg):
            lists(**kw)
    for kw, msg in (({"Kf": 0}, "Kf=0 outside"), ({"Kf": 33}, "Kf=33 outside"), ({"K": 65}, "K=65 outside"),
                    ({"consts": [float("nan"), rf2]}, "face constant 0 is not finite"), ({"consts": [tf2, -1.0]}, "face constant 1 is not finite and positive"),
                    ({"colh": None}, "null collision constants"), ({"flist_entries": n * 32 - 1}, "face lists of"), ({"flist_rows": n - 1}, "face lists of"),
                    ({"fdiag_rows": 0}, "fdiag of 0 rows"), ({"faces": None}, "null faces"), ({"block": 96}, "block=96"), ({"substeps": -1}, "substeps=-1"),
                    ({"fdiag": None}, "null diag / fdiag / fcsr"), ({"flist_f": None}, "null list / corr"),
                    ({"nf": (2 ** 31 - 1) // 3}, "faces: the table must stay below 2\\^31")):
        with pytest.raises(ValueError, match=msg):
            solver(**kw)
    torch.cuda.synchronize()
    assert torch.equal(t["x"], before) and flag.item() == 0 and not fc["fdiag"].any() and not fc["list_n"].any() and not c["diag"].any()
    assert ops.cloth_face_contact_lists([], device=DEV) == []


def test_a_bad_face_index_is_flagged_and_never_dereferenced(darts):
    start, variants = darts
    good = variants["R2"][0]
    faces = np.array(FC.DART_FACES)
    faces[1, 2] = 6                                                  # one past the last vertex
    broken = FC.dart(faces=faces, check=False)[0]
    assert broken.bad_index and broken.face_collision == good.face_collision
    with pytest.raises(IndexError):
        ops.cloth_face_contact_lists([good, broken], device=DEV)
    with pytest.raises(IndexError):
        ops.cloth_simulate_batch([good, broken], 4, states=[start, None], device=DEV)
    gs = [good, broken]
    dev = torch.device(DEV)
    col, fcol = ops.cloth_collision_constants(gs, "test"), ops.cloth_face_collision_constants(gs, "test")
    for lds in (24 * 6, 0):
        t = ops.cloth_device_tables(gs, [start, cloth.state_arrays(broken, None, None)], dev)
        c = ops.cloth_contact_buffers(gs, t, col, dev)
        fc = ops.cloth_face_buffers(gs, t, fcol, dev, chunks=3)
        n, pad, Kf = t["total_verts"], 8, fcol["Kf"]
        bufs = {}
        for k, src, width, dtype, fill in (("x", t["x"], 3, torch.float64, 7.25), ("v", t["v"], 3, torch.float64, 7.25),
                                            ("corr", c["corr"], 3, torch.float64, 7.25), ("list_f", fc["list_f"], Kf, torch.int32, 77),
                                            ("list_tm2", fc["list_tm2"], Kf, torch.float64, 7.25)):
            bufs[k] = (torch.full((n + 2 * pad, width), fill, dtype=dtype, device=DEV), fill)
            bufs[k][0][pad:pad + n] = src
        t["x"], t["v"], c["corr"] = (bufs[k][0][pad:pad + n] for k in ("x", "v", "corr"))
        fc["list_f"], fc["list_tm2"] = bufs["list_f"][0][pad:pad + n], bufs["list_tm2"][0][pad:pad + n]
        flag = torch.zeros(1, dtype=torch.int64, device=DEV)
        ops._cloth_lists_call(t, c, col, 2, _lib.CLOTH_LISTS_BUILD)
        ops._cloth_face_lists_call(t, fc, col, fcol, 2, flag)
        assert flag.item() == 1
        want = cloth.face_contact_lists_reference(good, start[0])
        assert np.array_equal(fc["list_f"][:6].cpu().numpy(), want[0][0]) and np.array_equal(fc["list_tm2"][:6].cpu().numpy(), want[0][1])
        assert want[1].sum() == 3, "the dart's vertices hold the big face"
        flag.zero_()
        _lib.call("gn_cloth_simulate_face_contacts_batch", ops._p(t["x"]), ops._p(t["v"]), ops._p(t["w"]), ops._p(t["pairs"]), ops._p(t["l0"]),
                  ops._p(t["alpha_t"]), ops._p(t["csr"]), ops._p(t["colour_off"]), 2, n, t["total_constraints"], 2, 50,
                  ctypes.cast(t["consts"], ctypes.c_void_p), lds, 64, ops._p(flag), ops._p(c["list_j"]), ops._p(c["list_tm2"]), ops._p(c["list_n"]),
                  col["K"], ctypes.cast(col["host"], ctypes.c_void_p), ops._p(c["corr"]), ops._p(c["diag"]), ops._p(fc["faces"]), ops._p(fc["fcsr"]),
                  fc["total_faces"], ops._p(fc["list_f"]), ops._p(fc["list_tm2"]), fc["list_f"].numel(), ops._p(fc["list_n"]), fc["list_n"].numel(), Kf,
                  ctypes.cast(fcol["host"], ctypes.c_void_p), ops._p(fc["fdiag"]), 2, ops._stream())
        assert flag.item() == 1
        with pytest.raises(IndexError):
            ops._raise_bad_face(flag.item(), "cloth_simulate")
        for k, (buf, fill) in bufs.items():
            assert bool((buf[:pad] == fill).all()) and bool((buf[pad + n:] == fill).all()), (k, lds)
        assert bool(t["x"].isfinite().all())
        good_want = cloth.simulate_reference(good, 2, *start)
        assert torch.equal(t["x"][:6].cpu(), torch.from_numpy(good_want[0])) and torch.equal(t["v"][:6].cpu(), torch.from_numpy(good_want[1])), \
            "the good garment of the same launch"


# ------------------------------------------------------------------------------------------------ simulate, end to end
def test_simulate_with_face_contacts_on_the_device_equals_the_numpy_backend(tmp_path):
    meshes = [open_box_mesh(0, n=3), open_box_mesh(1, n=4, drop=1)]
    flags = ["--h", "0.004", "--duration", "0.4", "--damping", "2", "--alpha_stretch", "0", "--alpha_bend", "0.01", "--density", "0.25", "--gravity", "9.81",
             "--self_collision", "--collision_thickness", "0.3", "--collision_margin", "0.1", "--collision_rebuild", "3", "--collision_max_list", "64",
             "--collision_relax", "1.0", "--face_contacts", "--face_thickness", "0.1", "--face_max_list", "24"]
    stores = {}
    for backend in ("hip", "numpy"):
        stores[backend] = str(tmp_path / f"{backend}.zarr")
        keys = write_canonical_store(stores[backend], meshes)
        out = SIM.main(["--zarr_in", stores[backend], "--backend", backend, "--batch_size", "2"] + flags)
        assert out["written"] == 2 and out["substeps"] == 100 and out["summary_written"]
    a, b = (zarr_store.open_group(stores[k], create=False) for k in ("hip", "numpy"))
    for key in keys:
        x, y = a["samples"][key]["mesh"]["cloth_verts"][:], b["samples"][key]["mesh"]["cloth_verts"][:]
        assert x.dtype == np.float32 and np.array_equal(x, y) and np.abs(x).max() > 0.1
        ra, rb = (r["samples"][key]["mesh"].attrs["cloth_simulation"] for r in (a, b))
        assert ra == rb and ra["collision_rebuild"] == 3 and ra["face_contact_max_list"] > 0 and ra["face_max_list"] == 24 and ra["face_thickness"] == 0.1
        assert set(cloth.FACE_COLLISION_FIELDS) | set(cloth.FACE_CONTACT_STATS) <= set(ra)
    assert np.array_equal(a["summary"]["cloth_aabb_union"][:], b["summary"]["cloth_aabb_union"][:])
