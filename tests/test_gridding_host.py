"""CPU: the restatements and inputs of tests/gridding_reference.py are what they claim to be -- the boundary points separate the reference's fp32 index
maths from any other formulation, the out-of-range set holds the values the GPU tests count on, the scatter yardsticks propagate NaNs, the two tile-flag
formulations agree and follow the documented layout, and the exact statistics are exact."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import gridding_reference as R
from oracle import pipeline as P


# ------------------------------------------------------------------------------------------------ points
@pytest.mark.parametrize("case", [1, 2, 4])
def test_boundary_points_separate_fp32_from_fp64_index_maths(case):
    """an fp64 evaluation of the index formula lands in another cell than the reference's fp32 maths on some lattice point of every axis: a kernel
    that fused, reassociated or multiplied by a reciprocal would be caught by these inputs"""
    grid, lo, hi = R.CASES[case]
    for a in range(3):
        x = torch.from_numpy(R.lattice_axis(grid[a], lo[a], hi[a]))
        pts = torch.zeros(len(x), 3) + torch.tensor(lo)
        pts[:, a] = x
        ref = P.points_grid_idxs(pts, list(lo), list(hi), grid)[:, a]
        f64 = R.cell_idx_f64(pts, lo, hi, grid)[:, a]
        n = int((ref != f64).sum())
        print(f"case {case} axis {a}: fp64 index differs on {n} of {len(x)} lattice points")
        assert n >= 1
        assert int((ref - f64).abs().max()) == 1                                        # (one cell, never more: both are the same formula)
    pts = R.boundary_points(case)
    _, gi = R.r_flat_idx(pts, torch.zeros(len(pts), dtype=torch.int64), lo, hi, grid)
    assert bool((gi != R.cell_idx_f64(pts, lo, hi, grid)).any())

@pytest.mark.parametrize("case", [1, 2, 3, 4])
def test_case_points_hold_what_the_gpu_tests_count_on(case):
    grid, lo, hi = R.CASES[case]
    pts = R.case_points(case)
    assert pts.dtype == torch.float32 and pts.shape[1] == 3 and bool(torch.isfinite(pts).all())
    for a in range(3):
        col = pts[:, a].numpy()
        lat = R.lattice_axis(grid[a], lo[a], hi[a])
        for v in np.concatenate([lat, np.nextafter(lat, np.float32(np.inf)), np.nextafter(lat, np.float32(-np.inf))]):
            assert (col == v).any()
        assert (col == np.float32(3e9)).any() and (col == np.float32(-3e9)).any() and float(np.float32(3e9)) * (grid[a] - 1) > 2 ** 31
        assert ((col == 0) & np.signbit(col)).any()                                     # -0.0
        assert (col == np.float32(1e-45)).any() and (col == np.float32(-1e-45)).any() and np.float32(1e-45) > 0
        assert col.max() >= 1e15 and col.min() <= -1e15
        assert (col == np.nextafter(np.float32(lo[a]), np.float32(-np.inf))).any() and (col == np.nextafter(np.float32(hi[a]), np.float32(np.inf))).any()
        inside = (col >= np.float32(lo[a])) & (col <= np.float32(hi[a]))
        assert inside.sum() >= 200 and (~inside).sum() >= 20
    # the reference clamps through int64: no index of these points leaves the grid
    flat, gi = R.r_flat_idx(pts, R.batch_with_empty_middle(len(pts)), lo, hi, grid)
    assert int(flat.min()) >= 0 and int(flat.max()) < 3 * int(np.prod(grid)) and bool((gi >= 0).all()) and bool((gi < torch.tensor(grid)).all())


def test_nonfinite_points_and_batches():
    pts = R.nonfinite_points()
    for grid, lo, hi in R.CASES.values():
        scaled = (pts + (-torch.tensor(lo))) * ((torch.tensor(grid, dtype=torch.float32) - 1) / (torch.tensor(hi) - torch.tensor(lo)))
        assert bool((~torch.isfinite(scaled)).any(dim=1).all())                         # every row has a coordinate without a portable integer value
    assert bool(torch.isnan(pts).any()) and bool((pts == float("inf")).any()) and bool((pts == -float("inf")).any())
    for n in (1, 3, 4, 5, 257):
        b = R.batch_with_empty_middle(n)
        assert len(b) == n and bool((b[1:] >= b[:-1]).all()) and not bool((b == 1).any()) and int(b[0]) == 0 and (n == 1 or int(b[-1]) == 2)


# ------------------------------------------------------------------------------------------------ scatter
def test_scatter_restatement_on_ordinary_values():
    g = R._gen(0)
    N, C, cells = 300, 7, 40
    src, flat = torch.randn(N, C, generator=g), torch.randint(0, cells, (N,), generator=g).to(torch.int32)
    idx = flat.long()[:, None].expand(-1, C)
    for reduce, red in (("sum", "sum"), ("mean", "mean")):
        ref = torch.zeros(cells, C).scatter_reduce(0, idx, src, red, include_self=False)
        torch.testing.assert_close(R.r_scatter(src, flat, cells, reduce), ref, rtol=1e-5, atol=1e-6)
    exact = torch.zeros(cells, C, dtype=torch.float64).index_add_(0, flat.long(), src.double())
    assert torch.equal(R.r_scatter(src, flat, cells, "sum"), exact.float())
    prod = torch.ones(cells, C).scatter_reduce(0, idx, src, "prod", include_self=True)
    torch.testing.assert_close(R.r_scatter(src, flat, cells, "mul"), prod, rtol=1e-5, atol=1e-30)
    padded = R.r_scatter(torch.cat([src[:, :5], torch.zeros(N, 2)], 1), flat, cells, "mul", c_real=5)
    assert torch.equal(padded[:, :5], R.r_scatter(src, flat, cells, "mul")[:, :5]) and bool((padded[:, 5:] == 0).all())


@pytest.mark.parametrize("C,c_real", [(1, None), (40, None), (144, 137)])
def test_special_value_scenarios_are_laid_out_as_stated(C, c_real):
    cps = int(np.prod(R.SCATTER_GRID))
    src, flat, cells, names = R.scenario_points(R.SPECIAL_CELLS, C, c_real)
    assert cells[:4] == [0, cps - 1, 2 * cps, 3 * cps - 1] and len(set(cells)) == len(R.SPECIAL_CELLS) == len(names)
    assert not any(cps <= c < 2 * cps for c in cells)                                    # the middle garment stays empty
    assert src.shape == (sum(len(v) for _, v in R.SPECIAL_CELLS), C) and sorted(set(flat.tolist())) == sorted(cells)
    assert not bool(torch.isnan(src).any())
    if c_real is not None:
        assert bool((src[:, c_real:] == 0).all())
    real = src[:, :c_real]
    b = R.bits(real)
    for want in (0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 5e-39, -5e-39, 3.4e38, -3.4e38):
        assert bool((b == int(np.float32(want).view(np.int32))).any()), want
    # the interleaving leaves some cell's points out of order, and some cell holds only negative values
    assert bool((flat[1:] < flat[:-1]).any())
    mx = R.r_scatter(src, flat, 3 * cps, "max", c_real)
    assert bool((mx[cells[5], :1] == -0.25).all()) and bool((mx[cells[1], :1] == 1.5).all())
    # every reduction's yardstick on these cells is free of NaNs except where the values themselves make one (inf - inf, 0 * inf)
    assert not bool(torch.isnan(mx).any()) and not bool(torch.isnan(R.r_scatter(src, flat, 3 * cps, "min", c_real)).any())
    assert bool(torch.isnan(R.r_scatter(src, flat, 3 * cps, "sum", c_real)[cells[3], 0]))


@pytest.mark.parametrize("reduce", R.REDUCES)
def test_every_yardstick_propagates_nans_of_either_sign(reduce):
    cps = int(np.prod(R.SCATTER_GRID))
    src, flat, cells, names = R.scenario_points(R.NAN_CELLS, 5)
    assert bool((R.bits(src) == np.int32(-1)).any()) and bool((R.bits(src) == 0x7fc00000).any()) and bool((R.bits(src) == np.array(0xffc00000, np.uint32).view(np.int32)).any())
    ref = R.r_scatter(src, flat, 3 * cps, reduce)
    occupied = torch.zeros(3 * cps, dtype=torch.bool)
    occupied[cells] = True
    assert bool(torch.isnan(ref[occupied]).all()), [n for n, c in zip(names, cells) if not bool(torch.isnan(ref[c]).all())]
    assert bool((ref[~occupied] == (1 if reduce == "mul" else 0)).all())


def _enc_max(u):
    """csrc/device_prims.h gn_ord_enc_max on bit patterns (uint32)"""
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    return np.where(nan, np.uint32(0xffffffff), np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000))).astype(np.uint32)


def _enc_min(u):
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    return np.where(nan, np.uint32(0), np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000))).astype(np.uint32)


def _dec(e):
    return np.where(e >> 31 == 1, e & np.uint32(0x7fffffff), ~e).astype(np.uint32)


def _dec_inv(e):
    return np.where(e >> 31 == 1, e, ~e & np.uint32(0x7fffffff)).astype(np.uint32)


def test_order_codes_of_the_scatter_on_paper():
    """the arithmetic of the max / min scatter restated on bit patterns: an unsigned maximum over gn_ord_enc_max(x) (min: over ~gn_ord_enc_min(x)),
    decoded by gn_ord_dec (gn_ord_dec_inv), is amax (amin) with NaNs of either sign propagated, and no float has the code 0 of an empty cell"""
    vals = [w for _, ws in R.SPECIAL_CELLS + R.NAN_CELLS for w in ws]
    u = R._f32(vals).view(np.uint32)
    u = np.unique(np.concatenate([u, np.array([0, 0x80000000, 1, 0x80000001, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7f800001, 0xff800001,
                                               0x7fc00000, 0xffc00000, 0x7fffffff, 0xffffffff], dtype=np.uint32)]))
    emax, emin = _enc_max(u), ~_enc_min(u)
    assert emax.min() > 0 and emin.min() > 0                                             # a zero-filled cell still reads as empty
    x = u.view(np.float32)
    fin = ~np.isnan(x)
    assert np.array_equal(_dec(emax)[fin], u[fin]) and np.array_equal(_dec_inv(emin)[fin], u[fin])          # round trip, bit for bit
    assert np.isnan(_dec(emax)[~fin].view(np.float32)).all() and np.isnan(_dec_inv(emin)[~fin].view(np.float32)).all()
    order = np.argsort(x[fin], kind="stable")
    xs, a, b = x[fin][order], emax[fin][order].astype(np.int64), emin[fin][order].astype(np.int64)
    lt = xs[1:] > xs[:-1]                                                               # (-0 and +0 compare equal as floats: either may win)
    assert (np.diff(a)[lt] > 0).all() and (np.diff(b)[lt] < 0).all()
    assert (emax[~fin] == 0xffffffff).all() and (emin[~fin] == 0xffffffff).all()          # a NaN beats every number in both
    for _, ws in R.SPECIAL_CELLS + R.NAN_CELLS:
        w = R._f32(ws)
        cu = w.view(np.uint32)
        t = torch.from_numpy(w.copy())
        got_max = _dec(np.array([_enc_max(cu).max()], dtype=np.uint32)).view(np.float32)
        got_min = _dec_inv(np.array([(~_enc_min(cu)).max()], dtype=np.uint32)).view(np.float32)
        assert R.same_values(torch.from_numpy(got_max.copy()), t.amax(0, keepdim=True)) and R.same_values(torch.from_numpy(got_min.copy()), t.amin(0, keepdim=True))


def test_same_values_and_bits():
    nan = float("nan")
    a = torch.tensor([1.0, nan, 0.0, float("inf")])
    assert R.same_values(a, a.clone()) and not torch.equal(a, a.clone())
    assert not R.same_values(a, torch.tensor([1.0, 2.0, 0.0, float("inf")])) and not R.same_values(a, torch.tensor([1.0, nan, 0.0, 3e38]))
    assert R.same_values(torch.tensor([0.0]), torch.tensor([-0.0])) and not torch.equal(R.bits(torch.tensor([0.0])), R.bits(torch.tensor([-0.0])))


# ------------------------------------------------------------------------------------------------ statistics
def test_exact_stats_are_exact():
    g = R._gen(3)
    vol = torch.zeros(2, 3, 2, 2, 4)
    vol[0].view(-1, 4)[[0, 5, 11]] = (10.0 ** (6 * torch.rand(3, 4, generator=g) - 3)) * torch.where(torch.rand(3, 4, generator=g) < 0.5, -1.0, 1.0)
    vol[0, 0, 0, 1, 0], vol[0, 1, 0, 0, 0] = 1e30, -1e30                                  # a cancellation that a plain fp64 sum gets wrong
    vol[0, 2, 1, 0, 0] = 1.0
    s, q, a = R.exact_stats(vol)
    for b in range(2):
        for c in range(4):
            col = [Fraction(float(v)) for v in vol[b, ..., c].reshape(-1)]
            assert s[b, c] == float(sum(col)) and q[b, c] == float(sum(v * v for v in col)) and a[b, c] == float(sum(abs(v) for v in col))
    assert not np.any(s[1]) and not np.any(q[1]) and s[0, 0] == float(sum(Fraction(float(v)) for v in vol[0, ..., 0].reshape(-1)))


# ------------------------------------------------------------------------------------------------ tile flags
def test_tile_flag_layout_by_hand():
    """grid (5, 9, 17): 2 x 2 x 3 tiles of 4 x 8 x 8 along axes 0, 1, 2; cell (4, 0, 16) reaches planes 3..4 (both tiles of axis 0), rows 0..1 (tile 0 of
    axis 1) and columns 15..16 (tiles 1 and 2 of axis 2): flags (ty * 3 + tx) * 2 + tz = 2, 3, 4, 5 and nothing else"""
    grid = (5, 9, 17)
    flat = torch.tensor([(4 * 9 + 0) * 17 + 16 + 2 * 5 * 9 * 17], dtype=torch.int32)
    f = R.r_tile_flags(flat, 3, grid, 1)
    assert f.shape == (3, 12) and not f[0].any() and not f[1].any() and np.flatnonzero(f[2]).tolist() == [2, 3, 4, 5]
    assert R.n_tiles(grid) == [2, 2, 3] and R.n_tiles((4, 8, 8)) == [1, 1, 1] and R.n_tiles((12, 20, 36)) == [3, 3, 5]


@pytest.mark.parametrize("grid", [(4, 8, 8), (5, 9, 17), (12, 20, 36)])
def test_tile_flag_formulations_agree(grid):
    flat = R.tile_test_cells(grid)
    cps = int(np.prod(grid))
    assert not bool(((flat >= cps) & (flat < 2 * cps)).any()) and bool((flat < cps).any()) and bool((flat >= 2 * cps).any())
    cells = set(flat.tolist())
    G0, G1, G2 = grid
    for i in (0, G0 - 1):                                                                # the eight corners of garment 0
        for j in (0, G1 - 1):
            for k in (0, G2 - 1):
                assert (i * G1 + j) * G2 + k in cells
    for a, t in enumerate(R.TILE):                                                       # both sides of every tile border the grid has
        for v in (t - 1, t):
            if v < grid[a]:
                c = [G0 // 2, G1 // 2, G2 // 2]
                c[a] = v
                assert (c[0] * G1 + c[1]) * G2 + c[2] in cells
    prev = None
    for reach in (1, 2, 3, 4):
        f = R.r_tile_flags(flat, 3, grid, reach)
        assert np.array_equal(f, R.r_tile_flags_by_voxel(flat, 3, grid, reach))
        assert not f[1].any() and f[0].any() and f[2].any() and (prev is None or (f >= prev).all())
        prev = f
    if grid != (4, 8, 8):
        assert not R.r_tile_flags(flat, 3, grid, 1)[2].all()                             # (not everything is flagged: the comparison can fail both ways)
