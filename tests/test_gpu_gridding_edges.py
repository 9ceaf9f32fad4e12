"""GPU (-m gpu): the forward gridding kernels of csrc/grid.hip -- gn_grid_features, gn_grid_scatter_ex, gn_grid_stats, gn_grid_tile_flags -- held to the
plain restatements of tests/gridding_reference.py at cell boundaries, outside the bounds, on non-cubic grids, at every tail of the launch shapes and on
the special values of fp32 (signed zeros, infinities, denormals, the largest finite value, NaNs of either sign).

Index results, copied columns and the max / min / mul volumes are compared bit for bit or by value as stated in each test; sum / mean against the
project's rule fp32(fp64 sum) (/ count in fp32); the occupied-cell statistics against an exact sum with a bound derived from the kernel's arithmetic,
not measured (test_grid_stats_against_an_exact_sum).  The shapes are the smallest at which each branch and tail exists, not the workload's.

Mutation record (one-line, in-bounds changes to csrc/grid.hip, each built once and run against this file on an MI355X; every other test passed):
  * the unfixed max / min encoder (the parent commit)            -> the six max / min cases of test_grid_scatter_propagates_nans_of_either_sign
  * index scale as the reciprocal of the corner step              -> test_grid_features_on_cell_boundaries_..[4], .._tails_strides_and_flags[4, 5, 257]
  * corner = fmaf(cell, step, lc)                                 -> test_grid_features_on_cell_boundaries_..[4], .._tails_strides_and_flags[every N]
    (with bounds 0 .. 1 both are the same arithmetic -- the scale is an integer, lc adds nothing: only case 4 can tell, which is why it is there)
  * flag layout with the tiles of axes 0 and 1 exchanged          -> 10 of test_grid_tile_flags_against_brute_force (all but the single tile and (5, 9, 17) at
                                                                     reach 3 and 4, where every tile of an occupied garment is flagged), all four test_sparse_first_conv_.._on_non_cubic_grids
  * gn_grid_stats without the flush at a change of garment        -> all six test_grid_stats_against_an_exact_sum
  * mean / sum finalize leaving the count workspace as it is      -> test_grid_scatter_prezeroed_..[mean, sum]
  * mul filling its identity into the pad channels too            -> test_grid_scatter_special_values[mul-144-137], .._propagates_nans_..[mul-144-137], .._prezeroed_..[mul]
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import _lib, ops  # noqa: E402
import gridding_reference as R  # noqa: E402

DEV = "cuda:0"


def _sliced(t, left=2, right=3):
    """t [N][C] fp32 on the device as a column slice of a wider buffer (leading dimension C + left + right), copied bit for bit"""
    wide = torch.full((t.shape[0], t.shape[1] + left + right), 0x7fc00000, dtype=torch.int32)           # NaNs around it: reading past a row shows
    wide[:, left:left + t.shape[1]] = R.bits(t)
    return wide.to(DEV).view(torch.float32)[:, left:left + t.shape[1]]


def _salt(t, seed):
    """a few special bit patterns strewn over a tensor that a kernel only copies"""
    words = torch.tensor([-0.0, float("inf"), -float("inf"), 1e-45, -5e-39, 3.4e38, float("nan")], dtype=torch.float32)
    n = t.numel()
    at = torch.randperm(n, generator=R._gen(seed))[:min(n, 14)]
    t.view(-1)[at] = words[torch.arange(len(at)) % len(words)]
    return t


# ------------------------------------------------------------------------------------------------ 1. gn_grid_features
def _features(pts, grid, lo, hi, Cf, include_point, include_conf, seed):
    N = len(pts)
    g = R._gen(seed)
    feat = _salt(torch.randn(N, Cf, generator=g), seed)
    sim, conf = _salt(torch.randn(N, 3, generator=g), seed + 1), _salt(torch.rand(N, 3, generator=g), seed + 2)
    batch = R.batch_with_empty_middle(N)
    feat_d = _sliced(feat)
    assert feat_d.stride(0) > Cf
    got, flat = ops.grid_features(feat_d, pts.to(DEV), sim.to(DEV), conf.to(DEV), batch.to(DEV), lo, hi, grid, include_point, include_conf)
    ref, flat_ref = R.r_grid_features(feat, pts, sim, conf, batch, lo, hi, grid, include_point, include_conf)
    where = (grid, N, Cf, include_point, include_conf)
    assert flat.dtype == torch.int32 and np.array_equal(flat.cpu().numpy().astype(np.int64), flat_ref.numpy()), where         # cell indices: exact
    got = got.cpu()
    assert got.shape == ref.shape, where
    gb, rb = R.bits(got), R.bits(ref)
    assert torch.equal(gb[:, :Cf], rb[:, :Cf]), ("feat", where)
    c = Cf
    if include_point:
        assert torch.equal(gb[:, c:c + 3], rb[:, c:c + 3]), ("nocs - corner", where)
        assert torch.equal(gb[:, c + 3:c + 6], rb[:, c + 3:c + 6]), ("sim_pos", where)
        c += 6
    if include_conf:
        assert torch.equal(gb[:, c:c + 3], rb[:, c:c + 3]), ("conf", where)
    return flat_ref


@pytest.mark.parametrize("case", [1, 2, 3, 4])
def test_grid_features_on_cell_boundaries_and_outside_the_bounds(case):
    """every lattice point x_k = fl32(k * fl32((uc - lc) / (G - 1)) + lc) of every axis with both fp32 neighbours, points outside the bounds from one
    ulp to 1e15 (3e9 scales past int32), -0.0 and +-1e-45, and seeded generic points: flat_idx exact and every output column bit-equal to the
    reference's fp32 maths (oracle/pipeline.py points_grid_idxs / idxs_to_points).  B = 3 with the middle garment empty, feat a column slice."""
    grid, lo, hi = R.CASES[case]
    pts = R.case_points(case)
    flat_ref = _features(pts, grid, lo, hi, 3, True, True, case)
    _, gi = R.r_flat_idx(pts, torch.zeros(len(pts), dtype=torch.int64), lo, hi, grid)
    n64 = int((gi != R.cell_idx_f64(pts, lo, hi, grid)).any(dim=1).sum())
    print(f"case {case}: {len(pts)} points, {len(torch.unique(flat_ref))} cells; an fp64 evaluation of the formula would differ on {n64} points")
    assert case == 3 or n64 >= 1


@pytest.mark.parametrize("N", [1, 3, 4, 5, 257])
def test_grid_features_tails_strides_and_flags(N):
    """N around the four points a workgroup owns, Cf around the 64 lanes of the copy loop, all four combinations of the include flags, ldf > Cf"""
    for i, Cf in enumerate((1, 63, 64, 65, 131)):
        case = (1, 3, 4)[i % 3]
        grid, lo, hi = R.CASES[case]
        pts = R.case_points(case, seed=N + Cf)[:N].contiguous()
        for include_point in (True, False):
            for include_conf in (True, False):
                _features(pts, grid, lo, hi, Cf, include_point, include_conf, N * 1000 + Cf)


@pytest.mark.parametrize("case", [1, 2, 3, 4])
def test_grid_features_nonfinite_coordinates_stay_inside_the_volume(case):
    """NaN, +-inf and +-3e38 (infinite after the scaling): the reference has no portable answer, but no cell index may leave [0, B * cells) -- the
    scatter behind it trusts flat_idx.  Nothing is scattered from these rows."""
    grid, lo, hi = R.CASES[case]
    pts = R.nonfinite_points()
    N = len(pts)
    batch = R.batch_with_empty_middle(N)
    z = torch.zeros(N, 3, device=DEV)
    _, flat = ops.grid_features(torch.zeros(N, 2, device=DEV), pts.to(DEV), z, z, batch.to(DEV), lo, hi, grid)
    flat = flat.cpu().long()
    cps = int(np.prod(grid))
    print(f"case {case}: flat_idx of the non-finite rows in [{int(flat.min())}, {int(flat.max())}] of {3 * cps}")
    assert bool((flat >= 0).all()) and bool((flat < 3 * cps).all())


# ------------------------------------------------------------------------------------------------ 2. / 3. gn_grid_scatter_ex
def _scatter(src, flat, reduce, c_real=None, **kw):
    vol = ops.grid_scatter(_sliced(src, 1, 2), flat.to(DEV), R.SCATTER_B, R.SCATTER_GRID, reduce, c_real=c_real, **kw)
    assert vol.shape == (R.SCATTER_B,) + R.SCATTER_GRID + (src.shape[1],)
    return vol.reshape(-1, src.shape[1]).cpu()


def _untouched(got, cells, reduce, c_real):
    empty = torch.ones(got.shape[0], dtype=torch.bool)
    empty[cells] = False
    c_real = got.shape[1] if c_real is None else c_real
    if reduce == "mul":
        return bool((R.bits(got[empty][:, :c_real]) == R.bits(torch.ones(1))).all()) and bool((R.bits(got[:, c_real:]) == 0).all())
    return bool((R.bits(got[empty]) == 0).all()) and bool((got[:, c_real:] == 0).all())


@pytest.mark.parametrize("C,c_real", [(1, None), (40, None), (65, None), (144, 137)])
@pytest.mark.parametrize("reduce", R.REDUCES)
def test_grid_scatter_special_values(reduce, C, c_real):
    """one hand-built scenario per cell (gridding_reference.SPECIAL_CELLS: signed zeros, infinities against finites and against each other, denormals,
    only negative values, +-3.4e38 pairs, single points) on a (3, 5, 7) grid, B = 3 with the middle garment empty, occupied cells at the first and last
    cell of the volume and on both sides of the empty garment; src a column slice.  max / min: torch.scatter_reduce amax / amin, equal by value and
    bit for bit wherever the value is not a zero.  sum / mean: fp32(fp64 sum) (/ count in fp32), mul: the product in ascending point index from 1 --
    equal by value, a NaN that the values themselves make (inf - inf) counting as equal to a NaN.  Untouched cells: +0 (mul: 1, pads 0) bit for bit."""
    src, flat, cells, names = R.scenario_points(R.SPECIAL_CELLS, C, c_real, seed=C)
    got = _scatter(src, flat, reduce, c_real)
    ref = R.r_scatter(src, flat, got.shape[0], reduce, c_real)
    bad = [n for n, c in zip(names, cells) if not R.same_values(got[c], ref[c])]
    assert not bad, (reduce, bad)
    if reduce in ("max", "min"):
        assert torch.equal(got, ref)
        nz = ref != 0
        assert torch.equal(R.bits(got)[nz], R.bits(ref)[nz])
    else:
        assert R.same_values(got, ref)
    assert _untouched(got, cells, reduce, c_real)


@pytest.mark.parametrize("C,c_real", [(1, None), (65, None), (144, 137)])
@pytest.mark.parametrize("reduce", R.REDUCES)
def test_grid_scatter_propagates_nans_of_either_sign(reduce, C, c_real):
    """THE rule (DESIGN.md "Gridding"): a NaN of either sign in any point of a cell makes that cell's channel NaN under every reduction, as
    torch.scatter_reduce does -- before or after a finite value, alone, with all payload bits set (whose plain order code is the one an empty cell
    has) -- and leaves every other cell alone."""
    control = [R.SPECIAL_CELLS[5], R.SPECIAL_CELLS[9], ("finite pair", [4.0, -6.0])]
    src, flat, cells, names = R.scenario_points(R.NAN_CELLS + control, C, c_real, seed=C + 1)
    got = _scatter(src, flat, reduce, c_real)
    ref = R.r_scatter(src, flat, got.shape[0], reduce, c_real)
    real = C if c_real is None else c_real
    n = len(R.NAN_CELLS)
    dropped = [name for name, c in zip(names[:n], cells[:n]) if not bool(torch.isnan(got[c, :real]).all())]
    assert not dropped, (reduce, "cells whose NaN was dropped", dropped)
    assert bool(torch.isnan(ref[cells[:n], :real]).all())
    assert not bool(torch.isnan(got[cells[n:]]).any()) and R.same_values(got, ref)
    assert _untouched(got, cells, reduce, c_real)


# ------------------------------------------------------------------------------------------------ 4. prezeroed
def _collisions(N, C, c_real, grid, seed, spread=False):
    """N points over B = 3 garments (the middle one empty) in UNSORTED batch order, most of them on a few hot cells; |values| in 1e-3 .. 1e3 when spread"""
    g = R._gen(seed)
    cps = int(np.prod(grid))
    hot = torch.randint(0, cps, (6,), generator=g)
    cell = torch.where(torch.rand(N, generator=g) < 0.5, hot[torch.randint(0, 6, (N,), generator=g)], torch.randint(0, cps, (N,), generator=g))
    batch = 2 * torch.randint(0, 2, (N,), generator=g)
    src = torch.randn(N, C, generator=g)
    if spread:
        src = torch.sign(src) * 10.0 ** (6 * torch.rand(N, C, generator=g) - 3)
    src[:, c_real:] = 0
    return src, (batch * cps + cell).to(torch.int32), batch


@pytest.mark.parametrize("reduce", R.REDUCES)
def test_grid_scatter_prezeroed_equals_plain_and_leaves_the_count_zeroed(reduce):
    """the path the pipeline takes (zeroed_volume on a side stream): the same volume as the plain call, the count workspace all zero again afterwards
    (gn_grid_stats and the next scatter rely on it), pads zero"""
    grid, B, C, c_real = R.CASES[3][0], 3, 144, 137
    src, flat, _ = _collisions(257, C, c_real, grid, 5)
    src_d, flat_d = _sliced(src), flat.to(DEV)
    plain = ops.grid_scatter(src_d, flat_d, B, grid, reduce, c_real=c_real)
    vol0, cnt = ops.zeroed_volume(B, grid, C, DEV)
    got = ops.grid_scatter(src_d, flat_d, B, grid, reduce, prezeroed=(vol0, cnt), c_real=c_real)
    assert got.data_ptr() == vol0.data_ptr() and torch.equal(got, plain)
    assert int(cnt.abs().max()) == 0
    assert bool((got[..., c_real:] == 0).all()) and bool((plain[..., c_real:] == 0).all())
    ref = R.r_scatter(src, flat, B * int(np.prod(grid)), reduce, c_real)
    # (sum / mean too: a few dozen fp32 values of similar size add exactly in fp64, whatever the order)
    assert torch.equal(got.reshape(-1, C).cpu(), ref)


# ------------------------------------------------------------------------------------------------ 5. gn_grid_stats
def _grid_stats(vol, flat_d, B, cps):
    """gn_grid_stats called directly, as ops.grid_scatter(with_stats=True) does behind a scatter: a zeroed count workspace, uninitialised outputs"""
    C = vol.shape[-1]
    cnt = torch.zeros(B * cps, dtype=torch.int32, device=DEV)
    s, q = ops._stats_buffers(B, C, DEV, True)
    s.fill_(float("nan")); q.fill_(float("nan"))
    _lib.call("gn_grid_stats", ops._p(vol), ops._p(flat_d), flat_d.numel(), C, cps, B, ops._p(cnt), ops._p(s), ops._p(q), ops._stream())
    return s.cpu().numpy(), q.cpu().numpy(), cnt.cpu()


@pytest.mark.parametrize("C", [32, 144, 320])
@pytest.mark.parametrize("reduce", ["max", "mean"])
def test_grid_stats_against_an_exact_sum(reduce, C):
    """per-garment, per-channel sum and sum of squares of a scattered volume from its occupied cells, against math.fsum over the whole volume.

    Bound, derived and not measured: every occupied cell is added once, in fp64, to a register partial (sequential, <= n_occ additions per garment and
    channel) and the partials are added with fp64 atomics in any order (<= n_occ more); each addition errs by at most 2^-53 of a partial sum that never
    exceeds sum |v|, so |got - exact| <= 2 n_occ 2^-53 sum |v| = n_occ 2^-52 sum |v| (the squares likewise, with sum v^2; v * v is exact in fp64).
    C = 320 takes the channel loop past its 256 threads; N = 63 / 64 / 65 sit around the 64 points of a block; the batch vector is not sorted (the
    partials are flushed at every change of garment); the middle garment is empty and must read exactly 0; |values| span 1e-3 .. 1e3.
    Measured on an MI355X: see DESIGN.md "Gridding"."""
    grid, B = R.CASES[3][0], 3
    cps = int(np.prod(grid))
    worst = 0.0
    for N in (1, 63, 64, 65, 1000):
        src, flat, batch = _collisions(N, C, C, grid, N + C, spread=True)
        assert N < 63 or bool((batch[1:] < batch[:-1]).any())                            # not sorted
        flat_d = flat.to(DEV)
        vol = ops.grid_scatter(src.to(DEV), flat_d, B, grid, reduce)
        s, q, cnt = _grid_stats(vol, flat_d, B, cps)
        occ = torch.zeros(B * cps, dtype=torch.bool)
        occ[flat.long()] = True
        assert torch.equal(cnt != 0, occ)                                                # every occupied cell was claimed once, no other
        n_occ = occ.reshape(B, cps).sum(1).numpy()
        assert n_occ[1] == 0 and not s[1].any() and not q[1].any()                       # the empty garment: exact zeros
        es, eq, ea = R.exact_stats(vol)
        bound_s, bound_q = n_occ[:, None] * 2.0 ** -52 * ea, n_occ[:, None] * 2.0 ** -52 * eq
        err_s, err_q = np.abs(s - es), np.abs(q - eq)
        rel = max(float((err_s / np.maximum(ea, 1e-300)).max()), float((err_q / np.maximum(eq, 1e-300)).max())) / 2.0 ** -52
        worst = max(worst, rel)
        print(f"[grid-stats] {reduce} C={C} N={N}: occupied cells {n_occ.tolist()}, max |sum - exact| {err_s.max():.3e} (bound {bound_s.max():.3e}), "
              f"max |sumsq - exact| {err_q.max():.3e} (bound {bound_q.max():.3e}), worst error {rel:.3f} x 2^-52 of sum|v|")
        assert bool((err_s <= bound_s).all()) and bool((err_q <= bound_q).all()), (reduce, C, N)
        if N == 1:                                                                       # one cell: nothing to round
            assert np.array_equal(s, es) and np.array_equal(q, eq)
    print(f"[grid-stats] {reduce} C={C}: measured maximum {worst:.3f} x 2^-52 x sum|v| (allowed: n_occ x 2^-52 x sum|v|)")


# ------------------------------------------------------------------------------------------------ 6. gn_grid_tile_flags
@pytest.mark.parametrize("grid", [(4, 8, 8), (5, 9, 17), (12, 20, 36), (32, 32, 32)])
@pytest.mark.parametrize("reach", [1, 2, 3, 4])
def test_grid_tile_flags_against_brute_force(reach, grid):
    """the flag array equals the brute-force restatement (every occupied cell marks the tile of every output voxel within reach, clamped; layout
    (ty * tiles_x + tx) * tiles_z + tz with 4 x 8 x 8 tiles along axes 0, 1, 2) exactly: three different axis lengths, so no two axes can be swapped
    unnoticed; cells in every corner, on both sides of the tile borders and in the interior; B = 3 with an empty garment"""
    flat = R.tile_test_cells(grid)
    got = ops.grid_tile_flags(flat.to(DEV), 3, grid, reach).cpu().numpy()
    ref = R.r_tile_flags(flat, 3, grid, reach)
    assert got.shape == ref.shape and got.dtype == np.uint8
    assert np.array_equal(got, ref), (grid, reach, np.argwhere(got != ref)[:8].tolist())
    assert not got[1].any() and got[0].any() and got[2].any()


# ------------------------------------------------------------------------------------------------ 7. occupancy-aware convolutions on non-cubic grids
@pytest.mark.parametrize("aiw", [True, False])
@pytest.mark.parametrize("grid", [(20, 36, 24), (36, 16, 40)])
def test_sparse_first_conv_is_bit_identical_to_dense_on_non_cubic_grids(grid, aiw):
    """test_gpu_parity.py::test_sparse_first_conv_is_bit_identical_to_dense on grids with three different axis lengths (none a multiple of the tile in
    every axis): the oracle is the dense launch of the same layers, which does not read the flags -- a flag layout with two axes exchanged, invisible on
    a cube, would leave active tiles at their rest value here"""
    R.sparse_first_conv_case(grid, 4, aiw, DEV)
