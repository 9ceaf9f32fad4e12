"""GPU (-m gpu): the point and grid gradient kernels (csrc/grad.hip) at the tails, strides, ties, orders and geometries where they could be wrong
while tests/test_gpu_autograd.py stays green.  Same method and same rule as that file: the yardstick is torch autograd in fp64 on the CPU over a
plain-torch restatement (here the SPARSE ones of tests/test_autograd_host.py, proven equal to the dense ones there); selections are bit-exact;
weighted gradients stay within 4 x (torch-fp32 against fp64, measured in the same test) + 1 fp32 ulp of the largest gradient (tests/grad_reference.py::_check,
which prints the `[grad-error]` line before it asserts).  No tolerance here is a constant.  The production shapes are in
tests/test_gpu_autograd_fullsize.py.

Where a sum's terms are exactly reproducible in fp32 (sa_gather_bwd, knn_interpolate_bwd, grad_vol) the ORDER is asserted bit for bit against an
explicit numpy float32 loop in ascending element index; each such test first asserts on the CPU that the descending order gives other bits.

Operands.  The kernels are called directly (ops.*_bwd).  Every float operand a wrapper accepts with a padded row stride is handed over two ways:
"contiguous" -- rows of exactly C floats (where C is no multiple of 4 the operands' stride C already differs from the output's pad4(C)) -- and
"wide" -- a column slice of a wider buffer, every operand of a call at its own width and column offset, the surrounding columns NaN.  The two
results must have the same bits and hold no NaN.  Either way the rows sit at the head of a taller NaN buffer, so that a kernel that confuses
two READ strides reads NaN inside the buffer instead of memory beyond it.

Mutation record (MI355X; 13 one-line mutants of csrc/grad.hip, each built as a library of its own apart from the tree and run once against the
tests of this file named below.  Every run was chosen so that the mutant stays inside every buffer: a mutant that swaps a READ stride with the
output's WRITE stride was run on the "contiguous" layout only, where the operand's stride C is at most the output's pad4(C).  On the unchanged
library all tests of this file pass.)
    1. ordered_sum_kernel reading w.lst instead of w.sorted: fails test_sa_gather_bwd_sums_in_ascending_row_index,
       test_knn_interpolate_bwd_sums_in_ascending_element_index and test_trilinear_sample_bwd_grad_vol_sums_in_ascending_query_index.
    2. segment_max_bwd_kernel, ldi <-> ldgi: fails test_segment_max_bwd_tails_and_strides[C-contiguous] for C = 1, 63, 65, 127, 129, 257; C = 64 and
       256 pass as they must (C = pad4(C): the two strides are equal).
    3. segment_max_bwd_kernel, ldg <-> ldo: fails test_segment_max_bwd_tails_and_strides[C-wide] for all eight C.
    4. global_max_bwd_kernel, ldi <-> ldgi: fails test_global_max_pool_bwd_tails_and_strides[C-contiguous] for C = 1, 63, 65, 127, 129, 257 (64 and 256
       pass as in 2).
    5. global_max_bwd_kernel, ldg <-> ldo: fails test_global_max_pool_bwd_tails_and_strides[C-wide] for all eight C.
    6. grid scatter, lds <-> ldg (gsb_bid_kernel given ldg, gsb_select_kernel given lds): fails test_grid_scatter_bwd_tails_and_strides[C-max-contiguous]
       for C = 1, 63, 65, 127, 129, 257 (64 and 256 pass as in 2).
    7. knn_neighbours_kernel, j > pj -> j >= pj: fails test_knn_ties_forward_and_backward_choose_the_same_sources[k] for k = 2, 3, 4, 8, 9, 12 at its
       first assertion (the lexsort); k = 1 passes as it must (the first pass has no predecessor).
    8. knn_neighbours_kernel without the d == pd clause: fails the same six cases; k = 1 passes as it must.
    9. ordered_sum_kernel, e / div -> e: fails test_knn_interpolate_bwd_tails_and_strides (all eight C),
       test_knn_interpolate_bwd_sums_in_ascending_element_index and test_trilinear_sample_bwd_grad_vol_sums_in_ascending_query_index (run on these
       only: their grad_rows sit at the head of a buffer div times as tall, so the mutant's rows e are NaN inside it).
   10. gsb_select_kernel, ch < c_real -> ch < C: HARMLESS BY CONSTRUCTION, no test can fail and none did (the 47 grid scatter, padded-channel, hot
       selection, signed-zero and NaN tests run against it all pass).  gsb_bid_kernel bids for channels below c_real only, so for ch >= c_real
       win[owner][ch] keeps the memset's 0x7f7f7f7f, which no point index reaches (N < 2^31 - 1 is required, and 0x7f7f7f7f points x 4 bytes is
       beyond any device): `win == p` is false there with or without the clause, which is redundant in this kernel.  The same clause in
       gsb_spread_kernel (mean, sum) is NOT redundant; test_grid_scatter_bwd_padded_channels[*-mean, *-sum] holds it (pads exactly 0 under a
       non-zero grad_vol).
   11. global_max_bwd_kernel with the LDS fold removed (every row group keeps its own winner): fails
       test_global_max_pool_bwd_tails_and_strides[C-contiguous] for all eight C, test_hot_selections_5000_equal_values and
       test_signed_zeros_as_the_extreme_give_one_winner_with_the_stored_bits.
   12. tri_grad_query_kernel, (float)(D - 1) <-> (float)(W - 1): fails test_trilinear_sample_bwd_tails_and_strides (all eight C) and
       test_trilinear_sample_gradient_geometry[1x4x6, 5x1x3, 4x7x1, 1x1x5, 2x5x3, 3x4x6]; [2x2x2] passes as it must (D = W).
   13. gn_segment_max_bwd launching 64 threads with the channel loop's stride left at 256: fails
       test_segment_max_bwd_tails_and_strides[C-contiguous] for C = 65, 127, 129, 256, 257; C = 1, 63, 64 pass as they must (one pass of the loop).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import autograd as A, ops  # noqa: E402
from garmentnets_amd.components.pointnet2 import Segments  # noqa: E402
from test_autograd_host import s_global_max, s_knn, s_sa_gather, s_scatter, s_segment_max  # noqa: E402
from grad_reference import _check, _gen, r_sample  # noqa: E402
from test_gpu_autograd import DEV, _grads, _hip_grads  # noqa: E402
from test_gpu_pointnet2_any_input import _sqd  # noqa: E402

CHANNELS = [1, 63, 64, 65, 127, 129, 256, 257]
DESTS = [1, 3, 5, 255, 257, 1025]
LAYOUTS = ["contiguous", "wide"]


def _bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _operand(t, layout, k, tall=1):
    """t (rows, C) -> the same values on the GPU in `layout`; k numbers the operands of one call (each wide operand gets its own width and offset);
    tall: how many times the rows the buffer must hold (spare NaN rows, see the module docstring)"""
    t = t.detach().cpu().float()
    rows, C = t.shape
    off, width = (1 + 3 * k, C + 3 + 4 * k) if layout == "wide" else (0, C)
    buf = torch.full((tall * rows * (C + 16) // width + 2, width), float("nan"), dtype=torch.float32)
    buf[:rows, off:off + C] = t
    return buf.to(DEV)[:rows, off:off + C]


def _no_nan(*ts):
    return all(not bool(torch.isnan(t).any()) for t in ts)


def _spread(shape, seed):
    """normal values scaled over 13 binades: a sum of them in another order rounds differently with near certainty"""
    g = _gen(seed)
    return torch.randn(shape, generator=g) * torch.exp2(torch.randint(-6, 7, shape, generator=g).float())


# ------------------------------------------------------------------------------------------------ fp32 restatements of the ordered sums (numpy)
def _seq_sum(dest, coef, g, div, n_dest, reverse=False):
    """ordered_sum_kernel: out[dest[e]] = fl(out[dest[e]] + fl(coef[e] * g[e // div])) for e ascending (reverse: descending), in float32, by an
    explicit loop; coef None: the term is g[e // div]; dest[e] < 0: no destination"""
    g = np.ascontiguousarray(g, np.float32)
    out = np.zeros((n_dest, g.shape[1]), np.float32)
    order = range(len(dest) - 1, -1, -1) if reverse else range(len(dest))
    for e in order:
        j = int(dest[e])
        if j >= 0:
            term = g[e // div] if coef is None else g[e // div] * np.float32(coef[e])
            out[j] = out[j] + term
    assert out.dtype == np.float32
    return out


def _expected_order(dest, coef, g, div, n_dest):
    fwd, rev = _seq_sum(dest, coef, g, div, n_dest), _seq_sum(dest, coef, g, div, n_dest, reverse=True)
    assert not np.array_equal(fwd, rev), "the inputs do not tell the ascending order from the descending one"
    return torch.from_numpy(fwd)


def _knn_coef_np(nbr, d2):
    """knn_coef_kernel: w = 1 / max(d2, 1e-16) in fp32, the sum over the valid ranks in rank order, one division"""
    nbr, d2 = nbr.numpy(), d2.numpy().astype(np.float32)
    w = np.float32(1) / np.maximum(d2, np.float32(1e-16))
    wsum = np.zeros(len(nbr), np.float32)
    for r in range(nbr.shape[1]):
        wsum = np.where(nbr[:, r] >= 0, wsum + w[:, r], wsum).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        coef = np.where(nbr >= 0, w / wsum[:, None], np.float32(0)).astype(np.float32)
    return coef.reshape(-1)


def _tri_axis_np(q, size):
    """gn_tri_src_index + gn_tri_cell for one axis in fp32 -> (x0, weight of x0, weight of x0 + 1)"""
    q = q.astype(np.float32)
    x = ((np.float32(2) * q - np.float32(1)) + np.float32(1)) / np.float32(2) * np.float32(size - 1)
    x = np.minimum(np.float32(size - 1), np.maximum(x, np.float32(0)))
    x0 = np.floor(x)
    assert x.dtype == np.float32
    return x0.astype(np.int64), (x0 + np.float32(1)) - x, x - x0


def _tri_elements_np(query, dims):
    """tri_elements_kernel: query (B, M, 3) -> (keys, weights) of the (B M 8) corner elements; query component 0 indexes the LAST volume axis"""
    B, M, _ = query.shape
    D, H, W = dims
    qn = query.numpy().reshape(B * M, 3)
    (x0, wx0, wx1), (y0, wy0, wy1), (z0, wz0, wz1) = _tri_axis_np(qn[:, 0], W), _tri_axis_np(qn[:, 1], H), _tri_axis_np(qn[:, 2], D)
    b = np.arange(B * M) // M
    keys, wgt = np.empty((B * M, 8), np.int64), np.empty((B * M, 8), np.float32)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        xx, yy, zz = x0 + dx, y0 + dy, z0 + dz
        ok = (xx < W) & (yy < H) & (zz < D)
        keys[:, c] = np.where(ok, ((b * D + zz) * H + yy) * W + xx, -1)
        wgt[:, c] = ((wx1 if dx else wx0) * (wy1 if dy else wy0)) * (wz1 if dz else wz0)
    return keys.reshape(-1), wgt.reshape(-1)


# ------------------------------------------------------------------------------------------------ 2. tails, widths and strides
def _segmax_inputs(M, S, C, seed):
    g = _gen(seed)
    h = torch.relu(torch.randn(M * S, C, generator=g))
    h[1::S] = h[0::S]                                          # slot 1 repeats slot 0: ties (and the ReLU's exact zeros)
    slot = torch.randint(-1, 50, (M * S,), generator=g).to(torch.int32)
    if M > 2:
        slot[S:2 * S] = -1                                     # a centre with no valid slot
    return h, slot, torch.randn(M, C, generator=g)


def _segmax_call(h, slot, gout, M, S, layout):
    hd, sd = _operand(h, layout, 0), slot.to(DEV)
    out = ops.segment_max(hd, sd, M, S)
    return out, ops.segment_max_bwd(_operand(gout, layout, 1), _operand(out, layout, 2), hd, sd, M, S)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_segment_max_bwd_tails_and_strides(C, layout):
    S = 5
    for M in DESTS:
        h, slot, gout = _segmax_inputs(M, S, C, 100 + C)
        fwd64, (g64,) = _grads(lambda t: s_segment_max(t, slot, M, S), [h], gout, torch.float64)
        out, g = _segmax_call(h, slot, gout, M, S, layout)
        assert torch.equal(out.cpu(), fwd64.float()), (C, M)
        assert torch.equal(g.cpu(), g64.float()) and _no_nan(g), (C, M)
        if layout != "contiguous":
            out2, g2 = _segmax_call(h, slot, gout, M, S, "contiguous")
            assert _bits(out, out2) and _bits(g, g2), (C, M)


def _gpool_inputs(B, C, seed):
    """examples of 1, 15, 16, 17, 33 and 0 rows in rotation; the winner of channel ch is planted in the first row (ch % 3 == 0, the last row
    holding the same value: the lower index wins), in the last row (ch % 3 == 1) and in the last row whose index mod 16 is 15, again with the
    last row tied (ch % 3 == 2, examples of at least 16 rows)"""
    base = [1, 15, 16, 17, 33, 0]
    sizes = [base[(i + B) % 6] for i in range(B)]
    g = _gen(seed)
    h = torch.relu(torch.randn(sum(sizes), C, generator=g))
    want = []                                                  # (row, example, channel class) that must take the gradient
    o = 0
    for b, n in enumerate(sizes):
        if n:
            h[o, 0::3] = h[o + n - 1, 0::3] = 9.0
            h[o + n - 1, 1::3] = 9.0
            want += [(o, b, 0), (o + n - 1, b, 1)]
            if n >= 16:
                r = (n - 16) // 16 * 16 + 15
                h[o + r, 2::3] = h[o + n - 1, 2::3] = 9.0
                want.append((o + r, b, 2))
        o += n
    return sizes, h, torch.randn(B, C, generator=g), want


def _gpool_call(h, sizes, gout, layout):
    hd, seg = _operand(h, layout, 0), Segments(sizes, DEV)
    out = ops.global_max_pool(hd, seg.ptr, seg.num)
    return out, ops.global_max_pool_bwd(_operand(gout, layout, 1), _operand(out, layout, 2), hd, seg.ptr, seg.num)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_global_max_pool_bwd_tails_and_strides(C, layout):
    seen = set()
    for B in DESTS:
        sizes, h, gout, want = _gpool_inputs(B, C, 200 + C)
        seen |= set(sizes)
        fwd64, (g64,) = _grads(lambda t: s_global_max(t, sizes), [h], gout, torch.float64)
        out, g = _gpool_call(h, sizes, gout, layout)
        assert torch.equal(out.cpu(), fwd64.float()), (C, B)
        assert torch.equal(g.cpu(), g64.float()) and _no_nan(g), (C, B)
        gc = g.cpu()
        for row, b, cls in want:                               # the planted winners, without the restatement
            assert torch.equal(gc[row, cls::3], gout[b, cls::3]), (C, B, row, cls)
        if layout != "contiguous":
            out2, g2 = _gpool_call(h, sizes, gout, "contiguous")
            assert _bits(out, out2) and _bits(g, g2), (C, B)
    assert seen == {1, 15, 16, 17, 33, 0}


def _scatter_inputs(N, C, cells, seed):
    g = _gen(seed)
    src = torch.randn(N, C, generator=g)
    cell = torch.randint(0, cells, (N,), generator=g)
    if N >= 4:
        src[N // 2:N // 2 + N // 4] = src[:N // 4]            # equal rows in equal cells: ties
        cell[N // 2:N // 2 + N // 4] = cell[:N // 4]
    return src, cell.to(torch.int32), torch.randn(cells, C, generator=g)


def _scatter_call(src, cell, gout, cells, reduce, layout):
    sd, cd = _operand(src, layout, 0), cell.to(DEV)
    vol = ops.grid_scatter(sd, cd, 1, (cells,), reduce)
    return vol, ops.grid_scatter_bwd(gout.to(DEV).view(vol.shape), cd, src.shape[0], reduce, vol=vol, src=sd)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("reduce", ["max", "min", "mean", "sum"])
@pytest.mark.parametrize("C", CHANNELS)
def test_grid_scatter_bwd_tails_and_strides(C, reduce, layout):
    cells = 7
    for N in DESTS:
        src, cell, gout = _scatter_inputs(N, C, cells, 300 + C)
        fn = lambda s: s_scatter(s, cell.long(), cells, reduce)        # noqa: E731
        fwd64, (g64,) = _grads(fn, [src], gout, torch.float64)
        vol, g = _scatter_call(src, cell, gout, cells, reduce, layout)
        if reduce in ("max", "min"):
            assert torch.equal(vol.view(cells, C).cpu(), fwd64.float()), (C, N)
            assert torch.equal(g.cpu(), g64.float()), (C, N)
        else:
            _, (g32,) = _grads(fn, [src], gout, torch.float32)
            _check(f"grid_scatter_bwd[{reduce}, C={C}, N={N}]", g64, g32, g)
        assert _no_nan(g)
        if layout != "contiguous":
            vol2, g2 = _scatter_call(src, cell, gout, cells, reduce, "contiguous")
            assert _bits(vol, vol2) and _bits(g, g2), (C, N)


@pytest.mark.parametrize("reduce", ["max", "min", "mean", "sum"])
@pytest.mark.parametrize("C,c_real", [(4, 3), (68, 65), (140, 137)])
def test_grid_scatter_bwd_padded_channels(C, c_real, reduce):
    """c_real < C, as the gridding calls it (137 real channels in rows of 140): the pad channels of src are zeros and take NO gradient, whatever
    grad_vol holds there (here: non-zero numbers), and the real channels get what the operator on c_real channels alone gives"""
    N, cells = 257, 7
    src, cell, gout = _scatter_inputs(N, C, cells, 350 + C)
    src[:, c_real:] = 0.0
    gout[:, c_real:] = gout[:, c_real:].abs() + 0.5
    sd, cd = src.to(DEV), cell.to(DEV)
    vol = ops.grid_scatter(sd, cd, 1, (cells,), reduce, c_real=c_real)
    g = ops.grid_scatter_bwd(gout.to(DEV).view(vol.shape), cd, N, reduce, vol=vol, src=sd, c_real=c_real)
    assert float(g[:, c_real:].abs().max()) == 0.0 and _no_nan(g)
    fn = lambda s: s_scatter(s, cell.long(), cells, reduce)            # noqa: E731
    fwd64, (g64,) = _grads(fn, [src[:, :c_real].clone()], gout[:, :c_real].clone(), torch.float64)
    if reduce in ("max", "min"):
        assert torch.equal(vol.view(cells, C)[:, :c_real].cpu(), fwd64.float())
        assert torch.equal(g[:, :c_real].cpu(), g64.float())
    else:
        _, (g32,) = _grads(fn, [src[:, :c_real].clone()], gout[:, :c_real].clone(), torch.float32)
        _check(f"grid_scatter_bwd[{reduce}, C={C}, c_real={c_real}]", g64, g32, g[:, :c_real])


def _slot_table(rows, n_points, seed):
    slot = torch.randint(-1, n_points, (rows,), generator=_gen(seed)).to(torch.int32)
    slot[::7] = n_points - 1                                   # the last point is read often, the last destination of the last block
    return slot


def _sa_ref(slot, C, n_points, gout, dtype):
    """the gradient of the sparse restatement with respect to x (positions are data: zeros do)"""
    pos = torch.zeros(n_points, 3)
    centre = torch.zeros(slot.numel(), dtype=torch.int64)
    x = torch.zeros(n_points, C)
    return _grads(lambda t: s_sa_gather(t, pos.to(t.dtype), centre, slot, 1), [x], gout, dtype)[1][0]


@pytest.mark.parametrize("C", CHANNELS)
def test_sa_gather_bwd_tails_and_strides(C):
    rows = 900
    for n_points in DESTS:
        slot = _slot_table(rows, n_points, 400 + C)
        gout = torch.randn(rows, C + 3, generator=_gen(401 + C))
        g64, g32 = _sa_ref(slot, C, n_points, gout, torch.float64), _sa_ref(slot, C, n_points, gout, torch.float32)
        g = ops.sa_gather_bwd(_operand(gout, "contiguous", 1), slot.to(DEV), C, n_points)
        _check(f"sa_gather_bwd[C={C}, n={n_points}]", g64, g32, g)
        g2 = ops.sa_gather_bwd(_operand(gout, "wide", 1), slot.to(DEV), C, n_points)
        assert _bits(g, g2) and _no_nan(g, g2), (C, n_points)


def _knn_table(Nq, k, Ns, seed):
    """a synthetic neighbour table: min(k, Ns) distinct sources per query in ascending d2, -1 / 0 past them"""
    g = _gen(seed)
    m = min(k, Ns)
    nbr = torch.full((Nq, k), -1, dtype=torch.int32)
    d2 = torch.zeros(Nq, k)
    nbr[:, :m] = torch.rand(Nq, Ns, generator=g).argsort(1)[:, :m].to(torch.int32)
    d2[:, :m] = (torch.rand(Nq, m, generator=g) * 0.1 + 1e-4).sort(1).values
    return nbr, d2


def _knn_ref(nbr, d2, Ns, gout, dtype):
    x = torch.zeros(Ns, gout.shape[1])
    return _grads(lambda t: s_knn(t, nbr, d2), [x], gout, dtype)[1][0]


@pytest.mark.parametrize("C", CHANNELS)
def test_knn_interpolate_bwd_tails_and_strides(C):
    Nq, k = 301, 3
    for Ns in DESTS:
        nbr, d2 = _knn_table(Nq, k, Ns, 500 + C)
        gout = torch.randn(Nq, C, generator=_gen(501 + C))
        g64, g32 = _knn_ref(nbr, d2, Ns, gout, torch.float64), _knn_ref(nbr, d2, Ns, gout, torch.float32)
        g = ops.knn_interpolate_bwd(_operand(gout, "contiguous", 1, tall=k), nbr.to(DEV), d2.to(DEV), Ns)
        _check(f"knn_interpolate_bwd[C={C}, Ns={Ns}]", g64, g32, g)
        g2 = ops.knn_interpolate_bwd(_operand(gout, "wide", 1, tall=k), nbr.to(DEV), d2.to(DEV), Ns)
        assert _bits(g, g2) and _no_nan(g, g2), (C, Ns)


def _rows3(t, layout, k, tall=1):
    """grad_rows (B, M, C) in `layout`: the rows of all examples in one padded buffer, as the wrapper accepts them"""
    B, M, C = t.shape
    v = _operand(t.reshape(B * M, C), layout, k, tall)
    return v.as_strided((B, M, C), (M * v.stride(0), v.stride(0), 1), v.storage_offset())


def _sampler_ref(vol_cl, q, gout, dtype):
    """vol_cl (B, D, H, W, C) channel-last -> (forward, grad_vol channel-last, grad_query) of F.grid_sample"""
    fwd, (gv, gq) = _grads(r_sample, [vol_cl.permute(0, 4, 1, 2, 3), q], gout, dtype)
    return fwd, gv.permute(0, 2, 3, 4, 1), gq


@pytest.mark.parametrize("C", CHANNELS)
def test_trilinear_sample_bwd_tails_and_strides(C):
    B, dims = 2, (2, 3, 5)
    for M in DESTS:
        g = _gen(600 + C)
        vol = torch.randn(B, *dims, C, generator=g)
        q = torch.rand(B, M, 3, generator=g) * 1.4 - 0.2
        gout = torch.randn(B, M, C, generator=g)
        _, gv64, gq64 = _sampler_ref(vol, q, gout, torch.float64)
        _, gv32, gq32 = _sampler_ref(vol, q, gout, torch.float32)
        gv, gq = ops.trilinear_sample_bwd(_rows3(gout, "contiguous", 1, tall=8), vol.to(DEV), q.to(DEV), want_vol=True, want_query=True)
        _check(f"trilinear_sample_bwd grad_vol[C={C}, M={M}]", gv64, gv32, gv)
        _check(f"trilinear_sample_bwd grad_query[C={C}, M={M}]", gq64, gq32, gq)
        gv2, gq2 = ops.trilinear_sample_bwd(_rows3(gout, "wide", 1, tall=8), vol.to(DEV), q.to(DEV), want_vol=True, want_query=True)
        assert _bits(gv, gv2) and _bits(gq, gq2) and _no_nan(gv, gq, gv2, gq2), (C, M)


# ------------------------------------------------------------------------------------------------ 3. the order of every ordered sum, bit for bit
def test_sa_gather_bwd_sums_in_ascending_row_index():
    rows, n_points, C = 3000, 130, 70
    slot = _slot_table(rows, n_points, 700)
    gout = _spread((rows, C + 3), 701)
    want = _expected_order(slot.numpy(), None, gout[:, :C].numpy(), 1, n_points)
    for layout in LAYOUTS:
        g = ops.sa_gather_bwd(_operand(gout, layout, 1), slot.to(DEV), C, n_points)
        assert _bits(g, want), layout


def test_knn_interpolate_bwd_sums_in_ascending_element_index():
    Nq, k, Ns, C = 1000, 3, 90, 70
    nbr, d2 = _knn_table(Nq, k, Ns, 710)
    nbr[:, 2][::5] = -1                                        # some queries with two neighbours only
    d2[:, 2][::5] = 0.0
    d2[::9, 0] = 0.0                                           # d2 = 0: the clamp
    gout = _spread((Nq, C), 711)
    want = _expected_order(nbr.numpy().reshape(-1), _knn_coef_np(nbr, d2), gout.numpy(), k, Ns)
    for layout in LAYOUTS:
        g = ops.knn_interpolate_bwd(_operand(gout, layout, 1, tall=k), nbr.to(DEV), d2.to(DEV), Ns)
        assert _bits(g, want), layout


def _lattice_queries(B, M, dims, seed):
    g = _gen(seed)
    D, H, W = dims
    return torch.stack((torch.randint(0, W, (B, M), generator=g) / (W - 1), torch.randint(0, H, (B, M), generator=g) / (H - 1),
                        torch.randint(0, D, (B, M), generator=g) / (D - 1)), 2)


def test_trilinear_sample_bwd_grad_vol_sums_in_ascending_query_index():
    """Queries exactly on lattice points of a volume whose sizes - 1 are powers of two: the in-range corner weighs exactly 1 and the others
    exactly 0 (asserted on the CPU), so grad_vol[voxel] is the sequential fp32 sum of grad_rows over that voxel's queries in ascending query
    index -- the zero-weight terms of the neighbouring lattice points add +-0 and change nothing."""
    B, M, C, dims = 2, 600, 20, (5, 9, 3)
    q = _lattice_queries(B, M, dims, 720)
    keys, wgt = _tri_elements_np(q, dims)
    assert set(np.unique(wgt).tolist()) == {0.0, 1.0}
    lower = wgt.reshape(-1, 8)
    assert bool((lower[:, 0] == 1).all()) and bool((lower[:, 1:] == 0).all()) and bool((keys.reshape(-1, 8)[:, 0] >= 0).all())
    gout = _spread((B, M, C), 721)
    rows = gout.reshape(B * M, C).numpy()
    want = _expected_order(keys, wgt, rows, 8, B * int(np.prod(dims)))
    # the statement of the issue, word for word: the plain sum per voxel over its queries, ascending
    assert np.array_equal(want.numpy(), _seq_sum(keys.reshape(-1, 8)[:, 0], None, rows, 1, B * int(np.prod(dims))))
    vol = torch.zeros(B, *dims, C)
    for layout in LAYOUTS:
        gv, _ = ops.trilinear_sample_bwd(_rows3(gout, layout, 1, tall=8), vol.to(DEV), q.to(DEV), want_vol=True, want_query=False)
        assert _bits(gv.view(-1, C), want), layout


# ------------------------------------------------------------------------------------------------ 4. hot destinations (each runs once)
def test_hot_voxels_4000_queries_in_one_cell():
    B, C, dims, M = 1, 16, (8, 8, 8), 4000
    g = _gen(800)
    vol = torch.randn(B, *dims, C, generator=g)
    q = (torch.tensor([3.0, 4.0, 2.0]) + torch.rand(B, M, 3, generator=g)) / 7.0     # all inside the cell x 3..4, y 4..5, z 2..3
    gout = _spread((B, M, C), 801)
    keys, wgt = _tri_elements_np(q, dims)
    assert len(np.unique(keys)) == 8 and int((keys >= 0).sum()) == 8 * M              # eight voxels, 4000 elements each
    _, gv64, gq64 = _sampler_ref(vol, q, gout, torch.float64)
    _, gv32, gq32 = _sampler_ref(vol, q, gout, torch.float32)
    gv, gq = ops.trilinear_sample_bwd(gout.to(DEV), vol.to(DEV), q.to(DEV), want_vol=True, want_query=True)
    _check("hot voxels grad_vol", gv64, gv32, gv)
    _check("hot voxels grad_query", gq64, gq32, gq)
    # and the order: the same fp32 weights (gn_tri_weight's products restated) times grad_rows, added in ascending element index
    assert _bits(gv.view(-1, C), _expected_order(keys, wgt, gout.reshape(M, C).numpy(), 8, int(np.prod(dims))))


def test_hot_source_one_source_and_k_3():
    src_sizes, q_sizes, C, k = [1, 50], [2500, 100], 33, 3
    g = _gen(810)
    ps, pq = torch.rand(sum(src_sizes), 3, generator=g), torch.rand(sum(q_sizes), 3, generator=g)
    x, gout = torch.randn(sum(src_sizes), C, generator=g), _spread((sum(q_sizes), C), 811)
    sseg, qseg = Segments(src_sizes, DEV), Segments(q_sizes, DEV)
    nbr, d2 = (t.cpu() for t in ops.knn_neighbours(ps.to(DEV), sseg.ptr, pq.to(DEV), qseg.ptr, k))
    assert bool((nbr[:2500, 0] == 0).all()) and bool((nbr[:2500, 1:] == -1).all())
    fwd64, (g64,) = _grads(lambda t: s_knn(t, nbr, d2), [x], gout, torch.float64)
    _, (g32,) = _grads(lambda t: s_knn(t, nbr, d2), [x], gout, torch.float32)
    out, (gx,) = _hip_grads(lambda t: A.knn_interpolate(t, ps.to(DEV), pq.to(DEV), sseg, qseg, k), [x], gout)
    assert torch.allclose(out.cpu().double(), fwd64, rtol=1e-5, atol=1e-5)
    _check("hot source: one source, k = 3", g64, g32, gx)
    assert _bits(gx, _expected_order(nbr.numpy().reshape(-1), _knn_coef_np(nbr, d2), gout.numpy(), k, sum(src_sizes)))


def test_hot_source_within_every_querys_first_k():
    Ns, Nq, C, k = 200, 4000, 33, 3
    g = _gen(820)
    ps = torch.rand(Ns, 3, generator=g)
    pq = ps[17] + 0.004 * torch.randn(Nq, 3, generator=g)      # every query next to source 17
    x, gout = torch.randn(Ns, C, generator=g), _spread((Nq, C), 821)
    sseg, qseg = Segments([Ns], DEV), Segments([Nq], DEV)
    nbr, d2 = (t.cpu() for t in ops.knn_neighbours(ps.to(DEV), sseg.ptr, pq.to(DEV), qseg.ptr, k))
    assert bool((nbr == 17).any(1).all())
    fwd64, (g64,) = _grads(lambda t: s_knn(t, nbr, d2), [x], gout, torch.float64)
    _, (g32,) = _grads(lambda t: s_knn(t, nbr, d2), [x], gout, torch.float32)
    out, (gx,) = _hip_grads(lambda t: A.knn_interpolate(t, ps.to(DEV), pq.to(DEV), sseg, qseg, k), [x], gout)
    assert torch.allclose(out.cpu().double(), fwd64, rtol=1e-5, atol=1e-5)
    _check("hot source: in every query's first k", g64, g32, gx)
    assert _bits(gx, _expected_order(nbr.numpy().reshape(-1), _knn_coef_np(nbr, d2), gout.numpy(), k, Ns))


def test_hot_point_in_every_centres_ball():
    n, C, K = 4000, 21, 16
    g = _gen(830)
    pos = 0.05 * torch.rand(n, 3, generator=g)                 # the whole cloud inside every ball of radius 0.25: each centre's table is points 0..15
    seg = Segments([n], DEV)
    idx = A.fps(pos.to(DEV), seg, 0.5)
    cseg = Segments([ops.fps_count(n, 0.5)], DEV)
    nbr, _ = A.ball_table(pos.to(DEV), idx, 0.25, seg, cseg, K)
    x = torch.randn(n, C, generator=g)
    edges, slot, S = ops.sa_gather(x.to(DEV), pos.to(DEV), idx.to(torch.int32), nbr)
    slot = slot.cpu()
    # point 3 is read by EVERY centre, once: it is in every ball table, and the self-loop rule, which removes "point c" from centre c's table and
    # appends it in the last slot, leaves centre 3 with one copy as well
    per_centre = (slot.view(nbr.shape[0], S) == 3).sum(1)
    assert nbr.shape[0] == 2000 and bool((per_centre == 1).all()), per_centre.unique(return_counts=True)
    gout = _spread((slot.numel(), C + 3), 831)
    fn = lambda t: s_sa_gather(t, pos.to(t.dtype), idx.cpu(), slot, S)     # noqa: E731
    fwd64, (g64,) = _grads(fn, [x], gout, torch.float64)
    _, (g32,) = _grads(fn, [x], gout, torch.float32)
    assert torch.equal(edges[:, :C].cpu(), fwd64[:, :C].float())
    gx = ops.sa_gather_bwd(gout.to(DEV), slot.to(DEV), C, n)
    _check("hot point: in every centre's ball", g64, g32, gx)
    assert _bits(gx, _expected_order(slot.numpy(), None, gout[:, :C].numpy(), 1, n))


def test_hot_selections_5000_equal_values():
    n, C = 5000, 70
    h = torch.full((n + 40, C), 2.5)
    h[n:] = torch.randn(40, C, generator=_gen(840)).clamp(max=2.0)         # a second, ordinary example / cell
    gout = torch.randn(2, C, generator=_gen(841))
    sizes = [n, 40]
    fwd64, (g64,) = _grads(lambda t: s_global_max(t, sizes), [h], gout, torch.float64)
    out, g = _gpool_call(h, sizes, gout, "contiguous")
    assert torch.equal(out.cpu(), fwd64.float()) and torch.equal(g.cpu(), g64.float())
    assert torch.equal(g[0].cpu(), gout[0]) and float(g[1:n].abs().max()) == 0.0
    cell = torch.cat((torch.full((n,), 4), torch.full((40,), 1))).to(torch.int32)
    for reduce in ("max", "min"):
        src = h if reduce == "max" else -h
        gv = torch.randn(6, C, generator=_gen(842))
        fwd64, (g64,) = _grads(lambda s: s_scatter(s, cell.long(), 6, reduce), [src], gv, torch.float64)
        vol, g = _scatter_call(src, cell, gv, 6, reduce, "contiguous")
        assert torch.equal(vol.view(6, C).cpu(), fwd64.float()) and torch.equal(g.cpu(), g64.float()), reduce
        assert torch.equal(g[0].cpu(), gv[4]) and float(g[1:n].abs().max()) == 0.0, reduce


# ------------------------------------------------------------------------------------------------ 5. kNN ties
def _tie_cloud():
    """examples: a 5^3 lattice of spacing 1/8 with every fourth source duplicated (appended after the lattice), an empty example (no sources, no
    queries: interpolation from nothing is undefined), two sources (fewer than k for every k > 2), a 3^3 lattice.  Queries: lattice points (a
    source and its duplicate tie at d2 = 0, six face neighbours tie behind them), edge midpoints (2 sources tie, 4 with duplicates behind),
    face centres (4 tie) and cell centres (8 tie).  All coordinates are multiples of 1/16: every d2 is exact in fp32, ties are exact ties."""
    ax = torch.arange(5) / 8.0
    lat = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), 3).reshape(-1, 3)
    ex0 = torch.cat((lat, lat[::4]))
    ex2 = torch.tensor([[0.5, 0.5, 0.5], [0.25, 0.5, 0.5]])
    ax3 = torch.arange(3) / 8.0 + 0.125
    ex3 = torch.stack(torch.meshgrid(ax3, ax3, ax3, indexing="ij"), 3).reshape(-1, 3)

    def queries(pts, n):
        sel = pts[torch.randperm(len(pts), generator=_gen(len(pts)))[:n]]
        return torch.cat((sel, sel + torch.tensor([1 / 16, 0, 0]), sel + torch.tensor([0, 1 / 16, 1 / 16]), sel + 1 / 16))
    src = [ex0, ex0[:0], ex2, ex3]
    qry = [queries(lat, 40), ex0[:0], torch.tensor([[0.375, 0.5, 0.5], [0.375, 0.25, 0.0]]), queries(ex3, 15)]   # ex2's first query is equidistant
    return torch.cat(src), [len(s) for s in src], torch.cat(qry), [len(q) for q in qry]


def _lexsort_neighbours(ps, ssz, pq, qsz, k):
    nbr, d2 = np.full((len(pq), k), -1, np.int32), np.zeros((len(pq), k), np.float32)
    ps, pq = ps.numpy(), pq.numpy()
    so = np.concatenate(([0], np.cumsum(ssz)))
    qo = np.concatenate(([0], np.cumsum(qsz)))
    groups = set()
    for b in range(len(ssz)):
        s, e = int(so[b]), int(so[b + 1])
        for q in range(int(qo[b]), int(qo[b + 1])):
            d = _sqd(ps[s:e], pq[q])
            order = np.lexsort((np.arange(e - s), d))[:k]
            nbr[q, :len(order)] = s + order
            d2[q, :len(order)] = d[order]
            if len(order) == k and e - s > k:
                groups.add(int((d == d[order[-1]]).sum()))     # the size of the tie group the k-th neighbour belongs to
                if d[np.lexsort((np.arange(e - s), d))[k]] == d[order[-1]]:
                    groups.add(-1)                              # ... and the cut falls INSIDE a tie group
    return nbr, d2, groups


@pytest.mark.parametrize("k", [1, 2, 3, 4, ops.KNN_MAXK, ops.KNN_MAXK + 1, 12])
def test_knn_ties_forward_and_backward_choose_the_same_sources(k):
    ps, ssz, pq, qsz = _tie_cloud()
    assert 0 in ssz and min(s for s in ssz if s) < 3
    want_nbr, want_d2, groups = _lexsort_neighbours(ps, ssz, pq, qsz, k)
    assert -1 in groups and max(groups) >= 4                   # this k cuts through a tie group, and groups of 4 or more sources occur
    sseg, qseg = Segments(ssz, DEV), Segments(qsz, DEV)
    # 1. the repeated search
    nbr, d2 = (t.cpu() for t in ops.knn_neighbours(ps.to(DEV), sseg.ptr, pq.to(DEV), qseg.ptr, k))
    assert np.array_equal(nbr.numpy(), want_nbr) and np.array_equal(d2.numpy(), want_d2)
    # 2. the forward read exactly those sources: i.i.d. normal features, another tied neighbour is an O(1) miss
    g = _gen(900 + k)
    C = 45
    x, gout = torch.randn(len(ps), C, generator=g), torch.randn(len(pq), C, generator=g)
    fn = lambda t: s_knn(t, nbr, d2)                           # noqa: E731
    fwd64, (g64,) = _grads(fn, [x], gout, torch.float64)
    _, (g32,) = _grads(fn, [x], gout, torch.float32)
    hip = lambda t: A.knn_interpolate(t, ps.to(DEV), pq.to(DEV), sseg, qseg, k)     # noqa: E731
    out, (gx,) = _hip_grads(hip, [x], gout)
    assert torch.allclose(out.cpu().double(), fwd64, rtol=1e-5, atol=1e-5)
    # 3. the gradient
    _check(f"knn ties[k={k}]", g64, g32, gx)
    assert _bits(gx, _expected_order(nbr.numpy().reshape(-1), _knn_coef_np(nbr, d2), gout.numpy(), k, len(ps)))


# ------------------------------------------------------------------------------------------------ 6. sampler geometry
@pytest.mark.parametrize("dims", [(1, 4, 6), (5, 1, 3), (4, 7, 1), (1, 1, 5), (2, 2, 2), (2, 5, 3), (3, 4, 6)], ids=lambda d: "x".join(map(str, d)))
def test_trilinear_sample_gradient_geometry(dims):
    B, C, M = 2, 24, 400
    g = _gen(1000 + 100 * dims[0] + 10 * dims[1] + dims[2])
    vol = torch.randn(B, C, *dims, generator=g)
    q = torch.rand(B, M, 3, generator=g) * 1.6 - 0.3           # inside, and beyond both borders on every axis
    q[:, :30] = torch.randint(0, 2, (B, 30, 3), generator=g).float()      # exactly ON the borders: corners of the unit cube
    q[:, 30:60, 0] = 0.0
    q[:, 60:90, 1] = 1.0
    q[:, 90:120, 2] = torch.randint(0, 2, (B, 30), generator=g).float()
    assert bool((q < 0).any()) and bool((q > 1).any())
    gout = torch.randn(B, M, C, generator=g)
    fwd64, (gv64, gq64) = _grads(r_sample, [vol, q], gout, torch.float64)
    _, (gv32, gq32) = _grads(r_sample, [vol, q], gout, torch.float32)
    out, (gv, gq) = _hip_grads(A.grid_sample_points, [vol, q], gout)
    assert torch.allclose(out.cpu().double(), fwd64, rtol=1e-5, atol=1e-5)
    name = "x".join(map(str, dims))
    _check(f"sampler geometry {name} grad_vol", gv64, gv32, gv)
    _check(f"sampler geometry {name} grad_query", gq64, gq32, gq)
    assert _no_nan(gv, gq)
    D, H, W = dims
    for comp, size in enumerate((W, H, D)):                    # query component 0 indexes the last volume axis
        if size == 1:
            assert float(gq[:, :, comp].abs().max()) == 0.0, (dims, comp)
        else:
            assert float(gq[:, :, comp].abs().max()) > 0.0, (dims, comp)
    outside = ((q <= 0) | (q >= 1)).to(DEV)
    assert float(gq[outside].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 7. +-0 and NaN in selections (properties)
def _one_winner_with_the_outputs_bits(g, src, out_rows, key, gout, valid=None):
    """exactly one element per (destination, channel) has a non-zero gradient, that gradient is the destination's, and the element's bits are the
    stored output's.  g, src (E, C); out_rows, gout (nkeys, C); key (E,)"""
    g, src, out_rows = g.cpu(), src.cpu(), out_rows.cpu()
    nz = g != 0
    if valid is not None:
        assert not bool(nz[~valid].any())
    count = torch.zeros(gout.shape, dtype=torch.int64).index_add_(0, key, nz.to(torch.int64))
    occupied = torch.zeros(gout.shape[0], dtype=torch.bool)
    occupied[key if valid is None else key[valid]] = True
    assert torch.equal(count, occupied[:, None].expand_as(count).to(torch.int64))
    e, c = nz.nonzero(as_tuple=True)
    assert _bits(g[e, c], gout[key[e], c])
    assert _bits(src[e, c], out_rows[key[e], c])


def _signed_zero_rows(n, C, seed, sign):
    """values of one sign (sign = -1: all <= 0, so a zero is the maximum) with -0.0 and +0.0 scattered in every channel"""
    g = _gen(seed)
    v = sign * (torch.rand(n, C, generator=g) + 0.1)
    z = torch.rand(n, C, generator=g)
    v[z < 0.15] = -0.0
    v[z > 0.85] = 0.0
    return v


def test_signed_zeros_as_the_extreme_give_one_winner_with_the_stored_bits():
    C = 70
    gout = torch.randn(6, C, generator=_gen(1100)).abs() + 0.5                  # non-zero
    # grid scatter, max (values <= 0) and min (values >= 0): six cells of 40 points
    cell = torch.arange(240) % 6
    for reduce, sign in (("max", -1.0), ("min", 1.0)):
        src = _signed_zero_rows(240, C, 1101, sign)
        for c in range(6):                                     # every (cell, channel) holds both zeros
            src[c, 0::2], src[c + 6, 0::2], src[c, 1::2], src[c + 6, 1::2] = -0.0, 0.0, 0.0, -0.0
        vol, g = _scatter_call(src, cell.to(torch.int32), gout, 6, reduce, "contiguous")
        assert float(vol.abs().max()) == 0.0
        _one_winner_with_the_outputs_bits(g, src, vol.view(6, C), cell, gout)
    # segment max: six centres of 40 slots, a few of them empty
    src = _signed_zero_rows(240, C, 1102, -1.0)
    key = torch.arange(240) // 40
    src[0::40, 0::2], src[1::40, 0::2], src[0::40, 1::2], src[1::40, 1::2] = -0.0, 0.0, 0.0, -0.0
    slot = torch.randint(0, 99, (240,), generator=_gen(1103)).to(torch.int32)
    slot[5::17] = -1
    out, g = _segmax_call(src, slot, gout, 6, 40, "contiguous")
    assert float(out.abs().max()) == 0.0
    _one_winner_with_the_outputs_bits(g, src, out, key, gout, slot >= 0)
    # global max pool: six examples of 40 rows (rows 0 and 1 sit in different row groups of the kernel, rows 0 and 16 in the same one)
    src[16::40] = src[0::40]
    out, g = _gpool_call(src, [40] * 6, gout, "contiguous")
    assert float(out.abs().max()) == 0.0
    _one_winner_with_the_outputs_bits(g, src, out, key, gout)


def _nan_property(g, src, key, gout):
    """no NaN element gets gradient, at most one element per (destination, channel) does, and every gradient is finite"""
    g, src = g.cpu(), src.cpu()
    assert bool(torch.isfinite(g).all())
    nz = g != 0
    assert not bool((nz & torch.isnan(src)).any())
    count = torch.zeros(gout.shape, dtype=torch.int64).index_add_(0, key, nz.to(torch.int64))
    assert int(count.max()) <= 1
    return count


def test_nan_among_numbers_never_takes_a_gradient():
    C = 70
    g0 = _gen(1110)
    gout = torch.randn(6, C, generator=g0).abs() + 0.5
    src = torch.randn(240, C, generator=g0)
    src[torch.rand(240, C, generator=g0) < 0.1] = float("nan")
    src[0] = float("nan")                                      # the first element of destination 0 (either layout) is a NaN in every channel
    clean = ~torch.isnan(src)
    cell = torch.arange(240) % 6
    for reduce in ("max", "min"):
        _, g = _scatter_call(src, cell.to(torch.int32), gout, 6, reduce, "contiguous")
        _nan_property(g, src, cell, gout)
    key = torch.arange(240) // 40
    assert bool(torch.zeros(6, C).index_add_(0, key, clean.float()).min() > 0)   # every (destination, channel) keeps a number
    slot = torch.zeros(240, dtype=torch.int32)
    _, g = _segmax_call(src, slot, gout, 6, 40, "contiguous")
    # the forwards of segment max and global max pool skip a NaN (fmaxf): the stored maximum is a number, and exactly one number takes the gradient
    assert int(_nan_property(g, src, key, gout).min()) == 1
    _, g = _gpool_call(src, [40] * 6, gout, "contiguous")
    assert int(_nan_property(g, src, key, gout).min()) == 1
