"""What the gridding suites share (test_gridding_host.py, test_gpu_gridding_edges.py, test_gpu_parity.py): the grids and bounds, the point sets that sit on
cell boundaries, and plain restatements of the forward gridding stage (cell index and aggregation features, the five scatter reductions, the
occupied-cell statistics, the tile occupancy flags).  numpy / torch on the CPU, written for clarity; a plain module, imported by its siblings; it holds
no test."""
import math

import numpy as np
import torch

from oracle import pipeline as P

# (grid, lower, upper): the smallest grids at which every branch and tail of the kernels exists -- a cube, the shipped 128-cube (indices only), a
# grid smaller than one tile in two axes with three different odd sizes, and a non-cubic grid with bounds that are not 0..1
CASES = {
    1: ((32, 32, 32), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    2: ((128, 128, 128), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    3: ((5, 9, 17), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    4: ((12, 20, 36), (-0.4, -0.4, -0.9), (0.4, 0.4, 0.05)),
}
TILE = (4, 8, 8)                                  # the output tile of the occupancy-aware convolution along axes 0, 1, 2
REDUCES = ("max", "mean", "sum", "min", "mul")
_F = np.float32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ points
def lattice_axis(G, lc, uc):
    """x_k = fl32(k * fl32((uc - lc) / (G - 1)) + lc), k = 0 .. G-1: where idxs_to_points puts the cell corners"""
    lc, uc = _F(lc), _F(uc)
    step = _F(_F(uc - lc) / _F(G - 1))
    return (np.arange(G, dtype=_F) * step).astype(_F) + lc


def boundary_axis(G, lc, uc):
    """the lattice points of one axis and both fp32 neighbours of each"""
    x = lattice_axis(G, lc, uc)
    return np.concatenate([x, np.nextafter(x, _F(np.inf)), np.nextafter(x, _F(-np.inf))]).astype(_F)


def out_of_range_axis(lc, uc):
    """both sides of [lc, uc] at distances from one ulp to 1e15 (3e9 * (G - 1) is past int32: the reference converts through int64 before it
    clamps), and the values around zero whose sign or size a shortcut could lose"""
    lc, uc = _F(lc), _F(uc)
    d = np.array([1e-6, 1e-3, 0.5, 1.0, 7.0, 1e3, 1e6, 3e9, 1e12, 1e15], dtype=_F)
    return np.concatenate([[np.nextafter(lc, _F(-np.inf)), np.nextafter(uc, _F(np.inf))], lc - d, uc + d, [3e9, -3e9],
                           [-0.0, 1e-45, -1e-45]]).astype(_F)


def _columns(cols, seed):
    """[n][3] from three per-axis value lists of different lengths: each list cycled to the longest and permuted on its own, so that every value of
    every axis appears and the axes are not aligned"""
    rng = np.random.default_rng(seed)
    n = max(len(c) for c in cols)
    return np.stack([rng.permutation(np.resize(c, n)) for c in cols], axis=1).astype(_F)


def case_points(case, n_generic=300, seed=0):
    """float32 [N][3]: boundary set + out-of-range set + seeded generic points (inside and a little outside the bounds), shuffled"""
    grid, lo, hi = CASES[case]
    edge = _columns([np.concatenate([boundary_axis(grid[a], lo[a], hi[a]), out_of_range_axis(lo[a], hi[a])]) for a in range(3)], seed)
    rng = np.random.default_rng(seed + 1)
    lo32, hi32 = np.array(lo, _F), np.array(hi, _F)
    generic = (lo32 + (hi32 - lo32) * rng.uniform(-0.05, 1.05, (n_generic, 3))).astype(_F)
    pts = np.concatenate([edge, generic])
    return torch.from_numpy(pts[rng.permutation(len(pts))])


def boundary_points(case, seed=0):
    grid, lo, hi = CASES[case]
    return torch.from_numpy(_columns([boundary_axis(grid[a], lo[a], hi[a]) for a in range(3)], seed))


def nonfinite_points():
    """rows that hold a NaN, an infinity, or +-3e38 (finite, infinite after the scaling) in every axis position, next to ordinary values"""
    bad = [float("nan"), float("inf"), -float("inf"), 3e38, -3e38]
    rows = [[v if a == k else 0.25 for a in range(3)] for v in bad for k in range(3)] + [[v, v, v] for v in bad] + [[float("nan"), float("inf"), -3e38]]
    return torch.tensor(rows, dtype=torch.float32)


def batch_with_empty_middle(n):
    """sorted batch vector over B = 3 garments whose middle one has no point (n = 1: garment 0 alone)"""
    return torch.cat([torch.zeros(n - n // 2, dtype=torch.int64), torch.full((n // 2,), 2, dtype=torch.int64)])


# ------------------------------------------------------------------------------------------------ cell index and features
def r_flat_idx(nocs, batch, lower, upper, grid):
    """the reference's index maths (fp32, truncation toward zero through int64, clamp) -> (flat [N] int64, cell [N][3] int64)"""
    gi = P.points_grid_idxs(nocs, list(lower), list(upper), tuple(grid))
    return ((batch * grid[0] + gi[:, 0]) * grid[1] + gi[:, 1]) * grid[2] + gi[:, 2], gi


def r_grid_features(feat, nocs, sim_pos, conf, batch, lower, upper, grid, include_point=True, include_conf=True):
    """-> (rows [N][Cf (+6) (+3)] fp32, flat [N] int64): feat | nocs - corner | sim_pos | conf"""
    flat, gi = r_flat_idx(nocs, batch, lower, upper, grid)
    cols = [feat]
    if include_point:
        cols += [nocs - P.idxs_to_points(gi, list(lower), list(upper), tuple(grid)), sim_pos]
    if include_conf:
        cols.append(conf)
    return torch.cat(cols, dim=1), flat


def cell_idx_f64(nocs, lower, upper, grid):
    """the same formula evaluated in fp64 from the same fp32 inputs: what a kernel that fused, reassociated or widened the arithmetic would compute"""
    lc, uc = torch.tensor(lower, dtype=torch.float32).double(), torch.tensor(upper, dtype=torch.float32).double()
    g = torch.tensor(grid, dtype=torch.float64)
    i = ((nocs.double() - lc) * ((g - 1) / (uc - lc))).to(torch.int64)
    return torch.minimum(torch.clamp(i, min=0), (g - 1).to(torch.int64))


def bits(t):
    """fp32 tensor -> its bit patterns (int32): equality that tells -0 from +0 and one NaN from another"""
    return t.contiguous().view(torch.int32)


def same_values(a, b):
    """torch.equal that also holds where both are NaN"""
    na, nb = torch.isnan(a), torch.isnan(b)
    z = torch.zeros((), dtype=a.dtype)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(torch.where(na, z, a), torch.where(nb, z, b))


# ------------------------------------------------------------------------------------------------ scatter
def r_scatter(src, flat, cells, reduce, c_real=None):
    """[cells][C] fp32.  max / min: torch.scatter_reduce (amax / amin).  sum / mean: the project's rule, fp32 of the fp64 sum, for mean divided by the
    count in fp32.  mul: the product in ascending point index from 1 (torch_scatter's CPU loop).  Untouched cells are 0; under mul they are 1 on the
    real channels and 0 on the pads [c_real, C)"""
    C = src.shape[1]
    c_real = C if c_real is None else c_real
    idx = flat.long()
    if reduce in ("max", "min"):
        return torch.zeros(cells, C).scatter_reduce(0, idx[:, None].expand(-1, C), src, {"max": "amax", "min": "amin"}[reduce], include_self=False)
    if reduce in ("sum", "add", "mean"):
        s = torch.zeros(cells, C, dtype=torch.float64).index_add_(0, idx, src.double()).float()
        if reduce == "mean":
            n = torch.zeros(cells).index_add_(0, idx, torch.ones(len(idx)))
            s = torch.where(n[:, None] > 0, s / n[:, None].clamp_min(1), s)
        return s
    assert reduce == "mul"
    out = torch.ones(cells, C)
    out[:, c_real:] = 0
    for p in range(src.shape[0]):
        out[int(idx[p])] = out[int(idx[p])] * src[p]
    return out


SCATTER_GRID, SCATTER_B = (3, 5, 7), 3
_NAN_POS, _NAN_NEG, _NAN_POS_FULL, _NAN_NEG_FULL = 0x7fc00000, 0xffc00000, 0x7fffffff, 0xffffffff


def _f32(words):
    """bit patterns or floats -> float32 array (ints are bit patterns)"""
    return np.array([np.array(w, np.uint32).view(_F) if isinstance(w, int) else _F(w) for w in words], dtype=_F)


SPECIAL_CELLS = [                                     # one scenario per cell: the values its points carry
    ("+0 and -0", [0.0, -0.0]),
    ("-inf and a finite", [-np.inf, 1.5]),
    ("+inf and a finite", [np.inf, -2.5]),
    ("+inf and -inf", [np.inf, -np.inf]),
    ("denormals of both signs", [1e-45, -1e-45, 5e-39, -5e-39]),
    ("all negative", [-1.0, -3.5, -0.25]),
    ("largest finite, twice", [3.4e38, 3.4e38]),
    ("most negative finite, twice", [-3.4e38, -3.4e38]),
    ("largest and most negative finite", [3.4e38, -3.4e38]),
    ("a single point", [-7.25]),
    ("a single denormal", [5e-39]),
    ("a single -0", [-0.0]),
]
NAN_CELLS = [
    ("+NaN then a finite", [_NAN_POS, 2.0]),
    ("a finite then +NaN", [-2.0, _NAN_POS]),
    ("-NaN then a finite", [_NAN_NEG, 2.0]),
    ("a finite then -NaN", [-2.0, _NAN_NEG]),
    ("+NaN only", [_NAN_POS]),
    ("-NaN only", [_NAN_NEG]),
    ("all-ones NaN only", [_NAN_NEG_FULL]),
    ("all-ones NaN among finites", [3.0, _NAN_NEG_FULL, -3.0]),
    ("largest +NaN among finites", [3.0, _NAN_POS_FULL, -3.0]),
    ("both NaNs", [_NAN_POS, _NAN_NEG]),
]


def scenario_cells(n):
    """flat indices of n occupied cells on SCATTER_GRID x SCATTER_B with garment 1 empty: the first cell, the last cell of garment 0, the first cell of
    garment 2, the last cell overall, then alternating between garments 0 and 2"""
    cps = int(np.prod(SCATTER_GRID))
    fixed = [0, cps - 1, 2 * cps, 3 * cps - 1]
    rest = [(7 + 11 * i) if i % 2 == 0 else (2 * cps + 5 + 13 * i) for i in range(n)]
    cells = (fixed + [c for c in rest if c not in fixed])[:n]
    assert len(set(cells)) == n and all(0 <= c < cps or 2 * cps <= c < 3 * cps for c in cells)
    return cells


def scenario_points(scenarios, C, c_real=None, seed=0):
    """-> (src [N][C] fp32, flat [N] int32, cells, names): scenario i's values in cell scenario_cells()[i]; channel ch sees the values rolled by ch, so
    every value takes every arrival position; the points of all cells interleaved by a seeded permutation; pads [c_real, C) are 0"""
    cells = scenario_cells(len(scenarios))
    rows, flat = [], []
    for cell, (_, words) in zip(cells, scenarios):
        v = _f32(words)
        k = len(v)
        rows.append(np.stack([np.roll(v, ch % k) for ch in range(C)], axis=1))       # [k][C]
        flat += [cell] * k
    src, flat = np.concatenate(rows), np.array(flat, dtype=np.int32)
    perm = np.random.default_rng(seed).permutation(len(flat))
    src, flat = src[perm], flat[perm]
    if c_real is not None:
        src[:, c_real:] = 0
    return torch.from_numpy(src.view(np.int32).copy()).view(torch.float32), torch.from_numpy(flat), cells, [n for n, _ in scenarios]


# ------------------------------------------------------------------------------------------------ occupied-cell statistics
def exact_stats(vol):
    """vol [B][..cells..][C] fp32 -> (sum, sum of squares, sum of |v|) [B][C] as Python floats rounded once from the exact value (math.fsum over the
    whole volume; the square of an fp32 value is exact in fp64)"""
    B, C = vol.shape[0], vol.shape[-1]
    v = vol.reshape(B, -1, C).double().cpu().numpy()
    s, q, a = np.zeros((B, C)), np.zeros((B, C)), np.zeros((B, C))
    for b in range(B):
        nz = np.flatnonzero(np.any(v[b] != 0, axis=1))                   # (zeros add nothing to an exact sum: skipped for speed, not for the value)
        for c in range(C):
            col = v[b, nz, c].tolist()
            s[b, c], q[b, c], a[b, c] = math.fsum(col), math.fsum(x * x for x in col), math.fsum(abs(x) for x in col)
    return s, q, a


# ------------------------------------------------------------------------------------------------ tile occupancy
def n_tiles(grid):
    return [-(-grid[a] // TILE[a]) for a in range(3)]


def r_tile_flags(flat, B, grid, reach):
    """uint8 [B][tiles]: every occupied cell marks the tile of every output voxel within `reach` of it (per axis, clamped to the grid); flag of tile
    (tz, ty, tx) along axes (0, 1, 2) at (ty * tiles_x + tx) * tiles_z + tz"""
    tz_n, ty_n, tx_n = n_tiles(grid)
    flags = np.zeros((B, tz_n * ty_n * tx_n), dtype=np.uint8)
    G0, G1, G2 = grid
    for c in np.asarray(flat, dtype=np.int64).tolist():
        w, h, d, b = c % G2, c // G2 % G1, c // (G2 * G1) % G0, c // (G2 * G1 * G0)
        for z in range(max(d - reach, 0), min(d + reach, G0 - 1) + 1):
            for y in range(max(h - reach, 0), min(h + reach, G1 - 1) + 1):
                for x in range(max(w - reach, 0), min(w + reach, G2 - 1) + 1):
                    flags[b, ((y // TILE[1]) * tx_n + x // TILE[2]) * tz_n + z // TILE[0]] = 1
    return flags


def r_tile_flags_by_voxel(flat, B, grid, reach):
    """the second formulation: every output voxel looks for an occupied cell in its (2 reach + 1)^3 window and, if there is one, marks its own tile"""
    tz_n, ty_n, tx_n = n_tiles(grid)
    G0, G1, G2 = grid
    occ = np.zeros((B, G0, G1, G2), dtype=bool)
    occ.reshape(-1)[np.asarray(flat, dtype=np.int64)] = True
    flags = np.zeros((B, ty_n, tx_n, tz_n), dtype=np.uint8)
    for b in range(B):
        for z in range(G0):
            for y in range(G1):
                for x in range(G2):
                    if occ[b, max(z - reach, 0):z + reach + 1, max(y - reach, 0):y + reach + 1, max(x - reach, 0):x + reach + 1].any():
                        flags[b, y // TILE[1], x // TILE[2], z // TILE[0]] = 1
    return flags.reshape(B, -1)


def tile_test_cells(grid, seed=0):
    """flat int32 indices over B = 3 (garment 1 empty): garment 0 holds the eight corners and both sides of every tile border that the grid has
    (3 | 4 on axis 0, 7 | 8 on axes 1 and 2); garment 2 holds the centre cell and a few seeded interior cells"""
    G = np.array(grid)
    corners = [[i * (G[0] - 1), j * (G[1] - 1), k * (G[2] - 1)] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    mid = (G // 2).tolist()
    borders = []
    for a in range(3):
        for v in (TILE[a] - 1, TILE[a]):
            if v < G[a]:
                c = list(mid)
                c[a] = v
                borders.append(c)
    g0 = np.unique(np.array(corners + borders), axis=0)
    rng = np.random.default_rng(seed)
    g2 = np.unique(np.concatenate([[mid], rng.integers(0, G, (3, 3))]), axis=0)
    cps = int(G.prod())
    flat = [(b * G[0] + c[:, 0]) * G[1] * G[2] + c[:, 1] * G[2] + c[:, 2] for b, c in ((0, g0), (2, g2))]
    out = np.concatenate(flat).astype(np.int32)
    assert out.min() >= 0 and out.max() < 3 * cps
    return torch.from_numpy(out[rng.permutation(len(out))])


# ------------------------------------------------------------------------------------------------ occupancy-aware first two convolutions
def sparse_first_conv_case(grid, mode, aiw, dev="cuda:0"):
    """the first TWO UNet convolutions behind a scattered volume (the encoder's first DoubleConv, 128 -> 128 -> 32) on a (G0, G1, G2) grid: the
    occupancy-aware launches must equal the dense launches of the same layers bit for bit (the epilogue statistics up to the order of their fp64
    atomics).  Occupied cells in corners / on faces / in the interior, a garment without any point.  Needs a GPU."""
    from garmentnets_amd import arith as AR, ops, synthetic as S
    from garmentnets_amd.components.unet3d import AtRest, DoubleConv
    DEV = dev
    G0, G1, G2 = grid = tuple(int(v) for v in grid)
    g = torch.Generator().manual_seed(G0)
    B, C = 3, 128
    cells = [torch.tensor([[0, 0, 0], [G0 - 1, G1 - 1, G2 - 1], [0, G1 - 1, 5], [G0 // 2, G1 // 2, G2 // 2], [G0 // 2, G1 // 2, G2 // 2 + 1], [3, 8, 9], [4, 7, 8]]),
             torch.zeros((0, 3), dtype=torch.int64),
             torch.randint(0, max(grid), (200, 3), generator=g) % torch.tensor(grid)]             # (on a cube: the draw itself)
    assert all(bool((c >= 0).all()) and bool((c < torch.tensor(grid)).all()) for c in cells)
    flat = torch.cat([(((b * G0 + c[:, 0]) * G1 + c[:, 1]) * G2 + c[:, 2]) for b, c in enumerate(cells)]).to(torch.int32)
    feats = torch.randn(flat.numel(), C, generator=g)
    vol, stats = ops.grid_scatter(feats.to(DEV), flat.to(DEV), B, grid, "max", with_stats=True)
    dc = DoubleConv(C, 32, encoder=True)                                   # 128 -> 128 -> 32, the shipped encoders.0
    dc.load_state_dict({k: S.synthetic_tensor("c." + k, tuple(v.shape), 1) for k, v in dc.state_dict().items()})
    dc = dc.to(DEV)
    # aiw: both layers in the affine-in-weights form (arith.affine_in_weights: per-sample weight packs + bias table, csrc/conv_prep.hip) --
    # the occupancy-aware launch must equal ITS dense launch bit for bit just the same
    a_sp = AR.DEFAULT.replace(conv_mode=mode, sparse_first_conv=True, affine_in_weights=aiw)
    a_dn = a_sp.replace(sparse_first_conv=False)
    y1_s, st1_s, sp2 = dc.SingleConv1.run_at_rest(vol, AtRest(flat.to(DEV), 1), stats, arith=a_sp)
    assert sp2.reach == 2 and sp2.small is not None and (sp2.value is not None) == aiw       # rest value reported <=> affine-in-weights ran
    y2_s, st2_s, _ = dc.SingleConv2.run_at_rest(y1_s, sp2, st1_s, arith=a_sp)
    both_s, _, both_rest = dc.run(vol, None, stats, None, sparse_flat=flat.to(DEV), arith=a_sp)
    assert (both_rest is not None) == aiw
    y1_d, st1_d, d2 = dc.SingleConv1.run_at_rest(vol, AtRest(flat.to(DEV), 1), stats, arith=a_dn)
    assert (d2 is not None) == aiw and (d2 is None or (d2.small is None and d2.value is not None))          # no small volume when dense
    # (layer 2's GroupNorm affine from the SAME statistics in both forms: the two launches' fp64 atomic sums agree to 1 ulp only, which
    #  once in a while lands on the other side of an fp32 rounding boundary of the affine -- that is the atomics' order, not the kernels)
    y2_d, st2_d, _ = dc.SingleConv2.run_at_rest(y1_d, d2, st1_s, arith=a_dn)
    if aiw:            # the garment without a point is at rest everywhere: every interior voxel of layer 1's output IS the rest value
        assert torch.equal(y1_d[1, 3, 4, 5], d2.value[1]) and torch.equal(y1_d[1, G0 // 2, G1 // 2, G2 // 2], d2.value[1])
    f1, f2 = ops.grid_tile_flags(flat.to(DEV), B, grid, 1), ops.grid_tile_flags(flat.to(DEV), B, grid, 2)
    a1, a2 = f1.sum(dim=1).tolist(), f2.sum(dim=1).tolist()
    print(f"grid={grid} mode={mode}: active tiles per garment, layer 1 {a1} / layer 2 {a2} of {f1.shape[1]}")
    assert a1[1] == 0 and a2[1] == 0 and 0 < a1[0] <= a2[0] < f1.shape[1] and bool((f2 >= f1).all())
    assert torch.equal(y1_s, y1_d) and torch.equal(y2_s, y2_d) and torch.equal(both_s, y2_d)
    # the statistics are fp64 atomic sums of identical per-tile fp32 partials: equal up to the order of the fp64 additions (1 ulp)
    for (s_s, q_s, _), (s_d, q_d, _) in ((st1_s, st1_d), (st2_s, st2_d)):
        assert float(((s_s - s_d).abs() / s_d.abs().clamp_min(1e-30)).max()) <= 1e-13 and float(((q_s - q_d).abs() / q_d.abs().clamp_min(1e-30)).max()) <= 1e-13
    assert bool(torch.isfinite(y2_s).all()) and float(y2_s.abs().max()) > 0
