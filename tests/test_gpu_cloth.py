"""GPU (-m gpu): the cloth solver of csrc/cloth.hip (ops.cloth_simulate_batch) against the numpy restatement of garmentnets_amd/cloth.py, bit for bit on
fp64 x and v (torch.equal, no tolerance), on both storage paths, at several workgroup sizes, in ragged batches and in chunked launches; the entry's
refusals; and `python -m garmentnets_amd.simulate` feeding prepare, the dataset and predict end to end.  tests/test_cloth_host.py holds the restatement
itself to the definition."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cloth_cases import PARAMS, TRIANGLE, TWO_TRIANGLES, garment, sheet, with_coincident, with_massless, write_canonical_store  # noqa: E402
from garmentnets_amd import _lib, cloth, ops  # noqa: E402
from garmentnets_amd import prepare as P  # noqa: E402
from garmentnets_amd import simulate as SIM  # noqa: E402
from garmentnets_amd.io import zarr_store  # noqa: E402
from garmentnets_amd.io.dataset import GarmentInputDataset  # noqa: E402
from test_winding_host import open_box_mesh  # noqa: E402

DEV = "cuda:0"
SUBSTEPS = 120
MESHES = {"triangle": (TRIANGLE, 0), "two_triangles": (TWO_TRIANGLES, 1), "5x4": (sheet(5, 4, seed=11), 7), "9x7": (sheet(9, 7, seed=12), 30),
          "massless": (with_massless()[:2], 2), "coincident": (with_coincident(), 0)}


@pytest.fixture(scope="module")
def cases():
    """name -> (garment, restatement after SUBSTEPS substeps as torch tensors), computed once and left unchanged"""
    out = {}
    for name, (mesh, grip) in MESHES.items():
        g = garment(mesh, grip=grip)
        out[name] = (g, tuple(torch.from_numpy(a) for a in cloth.simulate_reference(g, SUBSTEPS)))
    return out


def same(got, want, tag):
    assert got[0].dtype == got[1].dtype == torch.float64 and got[0].shape == want[0].shape, tag
    assert torch.equal(got[0].cpu(), want[0]), (tag, "x", (got[0].cpu() - want[0]).abs().max().item())
    assert torch.equal(got[1].cpu(), want[1]), (tag, "v", (got[1].cpu() - want[1]).abs().max().item())


@pytest.mark.parametrize("name", list(MESHES))
def test_device_equals_the_restatement(cases, name):
    g, want = cases[name]
    if name == "9x7":                                                # neither its constraint count nor any colour's size is a multiple of the workgroup's
        assert len(g.l0) % 64 and (np.diff(g.colour_off) % 64).all() and len(g.colour_off) > 8
    if name == "massless":
        assert g.n_massless == 2
    if name == "coincident":
        assert (g.l0 == 0).any()
    assert want[0].isfinite().all() and (want[0] - torch.from_numpy(g.x0)).abs().max() > 1e-3      # it moved, and stayed finite
    same(ops.cloth_simulate_batch([g], SUBSTEPS, block=64, device=DEV)[0], want, name)
    same(ops.cloth_simulate_batch([g], SUBSTEPS, device=DEV)[0], want, name + " (default block)")


def test_numpy_backend_is_the_restatement(cases):
    g, want = cases["5x4"]
    same(ops.cloth_simulate_batch([g], SUBSTEPS, backend="numpy")[0], want, "numpy backend")


def test_a_ragged_batch_equals_each_garment_alone(cases):
    names = ["triangle", "9x7", "5x4"]
    got = ops.cloth_simulate_batch([cases[n][0] for n in names], SUBSTEPS, block=128, device=DEV)
    for n, state in zip(names, got):
        same(state, cases[n][1], f"{n} in a batch of three")
        same(state, tuple(t.cpu() for t in ops.cloth_simulate_batch([cases[n][0]], SUBSTEPS, block=128, device=DEV)[0]), f"{n} alone")


def test_the_batch_offset_changes_nothing(cases):
    got = ops.cloth_simulate_batch([cases[n][0] for n in ("massless", "9x7", "two_triangles", "9x7")], SUBSTEPS, device=DEV)
    same(got[1], cases["9x7"][1], "9x7 at offset 1")
    same(got[3], cases["9x7"][1], "9x7 at offset 3")
    same(got[0], cases["massless"][1], "massless at offset 0")


def test_both_storage_paths_give_the_same_bits(cases):
    g, want = cases["9x7"]
    need = 24 * len(g.w)
    assert ops.cloth_storage_path(g) == "lds" and ops.cloth_storage_path(g, need) == "lds" and ops.cloth_storage_path(g, need - 1) == "global"
    in_lds = ops.cloth_simulate_batch([g], SUBSTEPS, lds_budget=need, block=64, device=DEV)[0]
    in_global = ops.cloth_simulate_batch([g], SUBSTEPS, lds_budget=need - 1, block=64, device=DEV)[0]
    no_lds = ops.cloth_simulate_batch([g], SUBSTEPS, lds_budget=0, block=256, device=DEV)[0]
    same(in_lds, want, "LDS path")
    same(in_global, want, "global path")
    same(no_lds, want, "global path, no LDS at all")
    assert torch.equal(in_lds[0], in_global[0]) and torch.equal(in_lds[1], in_global[1])


def test_a_batch_with_one_garment_on_each_path(cases):
    names = ["9x7", "5x4", "coincident"]
    gs = [cases[n][0] for n in names]
    budget = 24 * len(gs[1].w) + 8                                   # the 5 x 4 sheets fit, the 9 x 7 sheet does not
    assert [ops.cloth_storage_path(g, budget) for g in gs] == ["global", "lds", "lds"]
    for n, state in zip(names, ops.cloth_simulate_batch(gs, SUBSTEPS, lds_budget=budget, block=64, device=DEV)):
        same(state, cases[n][1], f"{n} under a budget of {budget} bytes")


@pytest.mark.parametrize("block", [64, 192, 1024])
def test_every_workgroup_size_gives_the_same_bits(cases, block):
    for n in ("9x7", "two_triangles"):
        same(ops.cloth_simulate_batch([cases[n][0]], SUBSTEPS, block=block, device=DEV)[0], cases[n][1], f"{n}, block {block}")
        same(ops.cloth_simulate_batch([cases[n][0]], SUBSTEPS, block=block, lds_budget=0, device=DEV)[0], cases[n][1], f"{n}, block {block}, global")


def test_two_hundred_substeps_equal_four_launches_of_fifty(cases):
    g = cases["9x7"][0]
    want = tuple(torch.from_numpy(a) for a in cloth.simulate_reference(g, 200))
    same(ops.cloth_simulate_batch([g], 200, max_substeps_per_launch=200, device=DEV)[0], want, "one launch of 200")
    same(ops.cloth_simulate_batch([g], 200, max_substeps_per_launch=50, device=DEV)[0], want, "four launches of 50")
    same(ops.cloth_simulate_batch([g], 200, max_substeps_per_launch=64, lds_budget=0, device=DEV)[0], want, "launches of 64, 64, 64, 8 on the global path")
    state = None
    for _ in range(4):                                               # four calls, x and v carried by the caller
        state = ops.cloth_simulate_batch([g], 50, states=None if state is None else [state], device=DEV)[0]
        state = tuple(t.cpu().numpy() for t in state)
    same(tuple(torch.from_numpy(a) for a in state), want, "four calls of 50")
    x0 = ops.cloth_simulate_batch([g], 0, device=DEV)[0]
    assert torch.equal(x0[0].cpu(), torch.from_numpy(g.x0)) and not x0[1].any()


def bad_garment():
    X, faces = sheet(3, 3, seed=13)
    faces = faces.copy()
    faces[2, 1] = 9                                                  # one past the last vertex
    faces[5, 0] = -1
    return cloth.garment(X, faces, 0, PARAMS, check=False)


def test_a_face_index_out_of_range_raises_and_writes_nothing_out_of_bounds(cases):
    bad = bad_garment()
    assert bad.bad_index
    with pytest.raises(IndexError, match="face index is out of bounds"):
        ops.cloth_simulate_batch([bad], 10, device=DEV)
    with pytest.raises(IndexError):
        ops.cloth_simulate_batch([bad], 0, device=DEV)               # the table is checked whatever the substep count
    # the entry itself, its x and v between guard rows: the good garments of the same launch are the restatement's, the guards stay
    gs = [cases["5x4"][0], bad, cases["triangle"][0]]
    for budget in (_lib.CLOTH_MAX_LDS, 0):
        t = ops.cloth_device_tables(gs, [cloth.state_arrays(g, None, None) for g in gs], torch.device(DEV))
        n, pad = t["total_verts"], 8
        bufs = {}
        for k in ("x", "v"):
            bufs[k] = torch.full((n + 2 * pad, 3), 7.25, dtype=torch.float64, device=DEV)
            bufs[k][pad:pad + n] = t[k]
        flag = torch.zeros(1, dtype=torch.int64, device=DEV)
        lds = max(24 * len(g.w) for g in gs) if budget else 0
        _lib.call("gn_cloth_simulate_batch", ops._p(bufs["x"][pad:]), ops._p(bufs["v"][pad:]), ops._p(t["w"]), ops._p(t["pairs"]), ops._p(t["l0"]),
                  ops._p(t["alpha_t"]), ops._p(t["csr"]), ops._p(t["colour_off"]), 3, n, t["total_constraints"], SUBSTEPS, 50,
                  ctypes.cast(t["consts"], ctypes.c_void_p), lds, 64, ops._p(flag), ops._stream())
        assert flag.item() == 1
        for k in ("x", "v"):
            assert bool((bufs[k][:pad] == 7.25).all()) and bool((bufs[k][pad + n:] == 7.25).all()), (k, budget)
        off = t["v_off"]
        for b, name in ((0, "5x4"), (2, "triangle")):
            got = tuple(bufs[k][pad + off[b]:pad + off[b + 1]] for k in ("x", "v"))
            same(got, cases[name][1], f"{name} beside a garment with a bad index, budget {budget}")
        assert bool(bufs["x"][pad + off[1]:pad + off[2]].isfinite().all())


def test_refusals(cases):
    g = cases["5x4"][0]
    x = g.x0.copy()
    x[3, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        ops.cloth_simulate_batch([g], 5, states=[(x, np.zeros_like(x))], device=DEV)
    with pytest.raises(ValueError, match="not finite"):
        ops.cloth_simulate_batch([g], 5, states=[(g.x0, np.full_like(x, np.inf))], device=DEV)
    with pytest.raises(ValueError, match="grip vertex 20 outside"):
        cloth.garment(*MESHES["5x4"][0], 20, PARAMS)
    for kw in ({"block": 100}, {"block": 2048}, {"lds_budget": _lib.CLOTH_MAX_LDS + 1}, {"max_substeps_per_launch": 0}, {"backend": "cpu"}):
        with pytest.raises(ValueError):
            ops.cloth_simulate_batch([g], 5, device=DEV, **kw)
    with pytest.raises(ValueError, match="substeps"):
        ops.cloth_simulate_batch([g], -1, device=DEV)
    other = cloth.garment(*MESHES["5x4"][0], 7, cloth.ClothParams(gravity=9.81, h=PARAMS.h / 2, damping=1.5, alpha_stretch=1e-7, alpha_bend=0.02, density=0.3))
    with pytest.raises(ValueError, match="share their step constants"):
        ops.cloth_simulate_batch([g, other], 5, device=DEV)
    # the entry's own limits, by name and before any launch
    t = ops.cloth_device_tables([g], [cloth.state_arrays(g, None, None)], torch.device(DEV))
    flag = torch.zeros(1, dtype=torch.int64, device=DEV)

    def entry(B=1, nv=None, nc=None, substeps=5, chunk=50, lds=0, block=64, consts=None):
        c = t["consts"] if consts is None else (ctypes.c_double * 6)(*consts)
        _lib.call("gn_cloth_simulate_batch", ops._p(t["x"]), ops._p(t["v"]), ops._p(t["w"]), ops._p(t["pairs"]), ops._p(t["l0"]), ops._p(t["alpha_t"]),
                  ops._p(t["csr"]), ops._p(t["colour_off"]), B, t["total_verts"] if nv is None else nv, t["total_constraints"] if nc is None else nc,
                  substeps, chunk, ctypes.cast(c, ctypes.c_void_p), lds, block, ops._p(flag), ops._stream())
    before = t["x"].clone()
    for kw, msg in (({"B": 65536}, "B=65536 outside"), ({"nv": 2 ** 31}, "below 2\\^31"), ({"nc": 2 ** 31}, "below 2\\^31"), ({"block": 96}, "block=96"),
                    ({"lds": 160 * 1024 + 8}, "lds_bytes="), ({"substeps": -2}, "substeps=-2"), ({"chunk": 0}, "max_substeps_per_launch=0"),
                    ({"consts": [float("nan"), 1, 0, 0, 0, 1]}, "step constant 0 is not finite")):
        with pytest.raises(ValueError, match=msg):
            entry(**kw)
    assert torch.equal(t["x"], before) and flag.item() == 0
    assert ops.cloth_simulate_batch([], 5, device=DEV) == []


# ------------------------------------------------------------------------------------------------ simulate, end to end
def test_simulate_feeds_prepare_the_dataset_and_predict(tmp_path):
    from garmentnets_amd import predict as PR
    meshes = [open_box_mesh(0, n=3), open_box_mesh(1, n=4, drop=1)]
    flags = ["--h", "0.004", "--duration", "0.4", "--damping", "2", "--alpha_stretch", "0", "--alpha_bend", "0.01", "--density", "0.25", "--gravity", "9.81"]
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
        assert ra == rb and ra["substeps"] == 100
    assert np.array_equal(a["summary"]["cloth_aabb_union"][:], b["summary"]["cloth_aabb_union"][:])
    din, dout = stores["hip"], str(tmp_path / "prediction.zarr")
    done = P.main(["--zarr_in", din, "--volume_size", "24", "--point_clouds", "--pc_img_size", "96", "--marching_cubes"])
    assert done["written"] == {"nocs_winding_number_field": 2, "sim_nocs_winding_number_field": 2, "point_cloud": 2, "marching_cube_mesh": 2}
    ds = GarmentInputDataset(din, num_pc_sample=1024, num_views=4, static_epoch_seed=True, enable_augumentation=False)
    assert len(ds) == 2 and ds[1] is not None
    PR.main(["--zarr_in", din, "--zarr_out", dout, "--num_pc_sample", "1024", "--num_views", "4", "--grid", "16", "--volume_size", "24", "--auto_level",
             "--static_epoch_seed", "--subset", "all"])
    assert len(zarr_store.open_group(dout, create=False)["samples"].keys()) == 2
