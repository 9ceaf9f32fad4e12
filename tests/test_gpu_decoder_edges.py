"""GPU (-m gpu): the implicit decoder's forward kernels (csrc/decode.hip) at the channel modes, row tails, geometries, values and launch sizes where
they could be wrong while tests/test_gpu_parity.py stays green.  The yardsticks are the plain restatements of tests/decoder_reference.py, proven on
the CPU in tests/test_decoder_reference_host.py:

  * the samplers (gn_trilinear_sample per query and brick, gn_trilinear_sample_batch, the sampler inside gn_implicit_decode) against tri_rows, a numpy
    float32 restatement that equals F.grid_sample on the CPU bit for bit: compared as BITS (a NaN equal to any NaN);
  * the fp32 decoder (gn_implicit_decode, gn_implicit_decode_batch) against a float64 evaluation, elementwise under decoder_fp32_bound, an a-priori
    rounding bound for any summation order (derived there, not fitted); every case prints its largest error / bound ratio.

How tight the decoder's yardsticks are.  decoder_fp32_bound is a worst case over summation orders and signs: 1e-2 .. 1e-1 of |y| on dense rows, of
which the kernel uses about 1e-3.  The fp64 comparison therefore catches gross errors only -- a lost partial sum, a swapped row, a wrong
stride (mutants 6, 7, 9) -- and is NOT a tight accuracy test.  The sensitive checks on the decoder are the bit identities: a pure function of the row,
the grid-stride loop against a call of its own, the in-kernel sampler against the sampler, the batch entry against the single call.

Operands.  Outputs, and xin where used, are handed over two ways, as in tests/test_gpu_autograd_edges.py: "contiguous" (rows of exactly C floats) and
"wide" (a column slice of a wider, taller NaN buffer, starting one row down).  The two results must have the same bits and the surrounding NaNs
must be untouched.  Wide column offsets keep the alignment the mode needs (4 floats where C % 4 == 0, 2 for other even C, 3 for odd C): no test
launches a misaligned pointer -- the misaligned calls of the last tests are refused by the library before any launch, which is what they assert.

Two rules are asserted here and stated in DESIGN.md ("Decoder forward kernels at their edges"): a NaN query component samples source index 0, and
the brick kernel turns an inf into a NaN exactly where the query's cell corner (x0, y0, z0) is +-inf and the query lies on an upper face.

Mutation record (MI355X; one-line mutants of csrc/decode.hip -- number 3 of device_prims.h, compiled into decode.hip's object only -- each built as
a library of its own apart from the tree and run once against the sampler tests of this file (1 - 5) or its decoder, gate and in-kernel sampler
tests (6 - 10), the tests that assert refusals left out.  Every mutant stays inside every buffer: it reorders, skips, or reads a row the buffer
holds.  On the unchanged library all 179 tests of this file pass.)
    1. tri_query, the three corner loops from 7 down to 0: fails test_sampler_channel_modes_and_row_tails (all 18 C, both layouts),
       test_quad_channels_on_a_row_stride_of_4n_plus_2_fall_to_the_8_byte_mode (all three), test_sampler_geometry[1x4x6, 5x1x3, 4x7x1, 2x2x2, 2x5x3] at
       every C, test_sampler_non_finite_voxels, test_sampler_batch[*-33-*], both per-query and batch NaN-query tests, and, because only one of two
       paths changed, test_in_kernel_sampler_is_the_sampler (all but 1x1x5 and 1x1x1) and test_brick_sampler_non_finite_voxels.  Geometries
       [1x1x5] and [1x1x1] pass as they must (at most two corners inside: the sum commutes), test_sampler_batch[*-1-*] passes too (one query per volume,
       on which the two orders happen to round alike), and test_brick_sampler as it must (the brick has its own loop).
    2. tri_query, the source index of component 0 taken with D and that of component 2 with W: fails the same tests, with geometry [1x1x5] failing and
       [2x2x2] and [1x1x1] passing as they must (D = W).
    3. gn_tri_cell, wx[0] <-> wx[1]: fails every per-query and batch sampler test of the file (99 cases), [1x1x1] included (the weight of its only
       corner becomes 0); test_brick_sampler passes as it must (the brick and the in-kernel sampler form their weights themselves).
    4. scalar mode, ch += 64 -> ch += 128: fails test_sampler_channel_modes_and_row_tails[65-contiguous, 65-wide] (channel 64 keeps its NaN);
       C = 1, 3, 5, 63 pass as they must (one pass of the loop).
    5. 16-byte mode, q += qpw -> q += 2 * qpw: fails test_sampler_channel_modes_and_row_tails[64-*, 128-*]; C = 4, 8, 16, 32 pass as they must (a wave
       holds at least its 8 queries at once: one pass of the loop).
    6. implicit_decode_kernel's row map, + 4 * h -> + 4 * (1 - h), in the store of the first hidden layer: fails
       test_decoder_fp32_against_fp64_under_the_rounding_bound (all 30), test_decoder_batch_entry_under_the_rounding_bound (all four), both grid-stride
       tests and test_decoder_is_a_pure_function_of_the_row (both).  The same change in BOTH places the map is written (the store and the partial sums
       of the last layer) is HARMLESS BY CONSTRUCTION and no test failed: the two swaps of rows r and r +- 4 cancel, every row is still its own function.
    7. the fold of the 8 partial sums, j < 8 -> j < 7: fails test_decoder_fp32_against_fp64_under_the_rounding_bound (all 30),
       test_decoder_batch_entry_under_the_rounding_bound (all four) and both grid-stride tests; test_decoder_is_a_pure_function_of_the_row and
       test_in_kernel_sampler_is_the_sampler pass as they must (both sides lose the same eighth).
    8. the tile loop's body run once: fails test_decoder_grid_stride_loop and test_decoder_batch_grid_stride_loop, nothing else (no other launch has more
       row tiles than workgroups).
    9. the xin loader, m * p.ldxin -> m * p.C0: fails test_decoder_fp32_against_fp64_under_the_rounding_bound[*-wide] (all 15) and
       test_decoder_batch_entry_under_the_rounding_bound (all four, in their wide half); every contiguous case passes as it must (ldxin = C0).
   10. the run_if test removed: fails test_run_if_gates_the_single_call[0.0, -0.0] and test_run_if_gates_each_row_set_of_the_batch_call; [1.0] passes as
       it must.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decoder_reference as R  # noqa: E402
from garmentnets_amd import ops  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
LAYOUTS = ["contiguous", "wide"]
SCALAR_C, PAIR_C, QUAD_C = [1, 3, 5, 63, 65], [2, 6, 12, 20, 24, 130, 256], [4, 8, 16, 32, 64, 128]
ROW_TAILS = [1, 7, 8, 9, 31, 32, 33, 257]
ids_dims = lambda d: "x".join(map(str, d))  # noqa: E731
ids_widths = lambda w: "-".join(map(str, w))  # noqa: E731


def _align(C):
    return 4 if C % 4 == 0 else 2 if C % 2 == 0 else 1


def _window(M, C, layout, a=None, lead=()):
    """-> (NaN buffer on the GPU, its [*lead][M][C] window, the window's index): the operand of one call in `layout`; a: floats the window's base
    and row stride must be a multiple of (default: what the sampler's mode for C needs)"""
    a = a or _align(C)
    if layout == "contiguous":
        shape, idx = lead + (M + 2, C), tuple(slice(None) for _ in lead) + (slice(0, M), slice(None))
        if lead:                                                        # (row sets packed back to back: no spare rows between them)
            shape, idx = lead + (M, C), tuple(slice(None) for _ in lead) + (slice(None), slice(None))
    else:
        off = 4 if a == 4 else 3 * a
        width = off + C + 5 * a
        shape, idx = lead + (M + 3, width), tuple(slice(None) for _ in lead) + (slice(1, 1 + M), slice(off, off + C))
        if lead:
            shape, idx = lead + (M, width), tuple(slice(None) for _ in lead) + (slice(None), slice(off, off + C))
    buf = torch.full(shape, NAN, dtype=torch.float32, device=DEV)
    return buf, buf[idx], idx


def _surroundings_untouched(buf, idx):
    b = buf.cpu().clone()
    b[idx] = NAN
    return bool(torch.isnan(b).all())


def _np(t):
    return t.detach().cpu().contiguous().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a, b):
    return R.same_bits(_np(a), _np(b))


def _sample(vol, q, M, C, layout, **kw):
    """gn_trilinear_sample into a window of `layout` -> its rows (numpy); asserts that nothing around the window was written"""
    buf, win, idx = _window(M, C, layout)
    got = ops.trilinear_sample(vol, query=q, out=win, **kw)
    assert got.data_ptr() == win.data_ptr()
    assert _surroundings_untouched(buf, idx), (M, C, layout)
    return _np(win)


# ------------------------------------------------------------------------------------------------ sampler: channel modes x row tails
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", SCALAR_C + PAIR_C + QUAD_C)
def test_sampler_channel_modes_and_row_tails(C, layout):
    vol = R.spread(R.BASE_DIMS + (C,), 11 + C)
    q = R.query_table(R.BASE_DIMS, n=max(ROW_TAILS), seed=C)
    want = R.tri_rows(vol, q)
    assert not np.isnan(want).any()
    vd, qd = _dev(vol), _dev(q)
    for M in ROW_TAILS:
        got = _sample(vd, qd[:M].contiguous(), M, C, layout)
        assert R.same_bits(got, want[:M]), (C, M, layout)


@pytest.mark.parametrize("C", [8, 32, 128])
def test_quad_channels_on_a_row_stride_of_4n_plus_2_fall_to_the_8_byte_mode(C):
    """C % 4 == 0 with ldo % 4 == 2: rows are only 8-byte aligned, the kernel must choose the 8-byte mode (same bits)"""
    vol, q = R.spread(R.BASE_DIMS + (C,), 11 + C), R.query_table(R.BASE_DIMS, n=257, seed=C)
    want = R.tri_rows(vol, q)
    buf = torch.full((260, C + 14), NAN, dtype=torch.float32, device=DEV)
    win = buf[2:259, 2:2 + C]
    assert win.stride(0) % 4 == 2 and win.data_ptr() % 8 == 0
    ops.trilinear_sample(_dev(vol), query=_dev(q), out=win)
    assert R.same_bits(_np(win), want) and _surroundings_untouched(buf, (slice(2, 259), slice(2, 2 + C)))


# ------------------------------------------------------------------------------------------------ sampler: geometry
@pytest.mark.parametrize("C", R.GEOMETRY_CHANNELS)
@pytest.mark.parametrize("dims", R.GEOMETRIES, ids=ids_dims)
def test_sampler_geometry(dims, C):
    """size-1 axes, the 2-voxel cell and an odd box, on every exact voxel coordinate, its fp32 neighbours, the border and far beyond it"""
    vol, q = R.spread(dims + (C,), 11 + C), R.query_table(dims, seed=C)
    want = R.tri_rows(vol, q)
    vd, qd = _dev(vol), _dev(q)
    for layout in LAYOUTS:
        assert R.same_bits(_sample(vd, qd, len(q), C, layout), want), (dims, C, layout)


# ------------------------------------------------------------------------------------------------ sampler: non-finite voxels, NaN queries
def _non_finite_volume(dims, C, seed):
    """channel 0 / 1 / 2 hold +inf / -inf / NaN at voxel (0, 0, 0), at the far corner and at one interior voxel of an otherwise random volume"""
    D, H, W = dims
    vol = R.spread(dims + (C,), seed)
    for z, y, x in ((0, 0, 0), (D - 1, H - 1, W - 1), (D // 2, H // 2, W // 2)):
        vol[z, y, x, 0], vol[z, y, x, 1], vol[z, y, x, 2] = np.inf, -np.inf, np.nan
    return vol


def _voxel_lattice(dims):
    """every voxel's own coordinate (weights exactly 0 and 1)"""
    D, H, W = dims
    ax = [np.arange(n, dtype=np.float32) / np.float32(max(n - 1, 1)) for n in (W, H, D)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(g, np.float32)


@pytest.mark.parametrize("C", [3, 24, 32])
def test_sampler_non_finite_voxels(C):
    vol = _non_finite_volume(R.BASE_DIMS, C, 40 + C)
    q = np.concatenate([_voxel_lattice(R.BASE_DIMS), R.query_table(R.BASE_DIMS, n=400, seed=C)])
    want = R.tri_rows(vol, q)
    assert np.isposinf(want).any() and np.isneginf(want).any() and np.isnan(want).any() and np.isfinite(want[:, :3]).any()
    for layout in LAYOUTS:
        assert R.same_bits(_sample(_dev(vol), _dev(q), len(q), C, layout), want), (C, layout)


def _nan_queries():
    q = np.array([[np.nan, 0.3, 0.7], [0.3, np.nan, 0.7], [0.3, 0.7, np.nan], [np.nan, np.nan, np.nan], [np.nan, 1.0, 1.0]], np.float32)
    return q, np.where(np.isnan(q), np.float32(0), q)


def test_nan_query_component_samples_source_index_0_per_query_sampler():
    vol = R.spread(R.BASE_DIMS + (24,), 3)
    q, z = _nan_queries()
    want = R.tri_rows(vol, q)
    assert R.same_bits(want, R.tri_rows(vol, z)) and not np.isnan(want).any()
    assert R.same_bits(_sample(_dev(vol), _dev(q), len(q), 24, "contiguous"), want)


def test_nan_query_component_samples_source_index_0_batch_sampler():
    vol = R.spread((2,) + R.BASE_DIMS + (24,), 4)
    q, _ = _nan_queries()
    got = ops.trilinear_sample_batch(_dev(vol), _dev(np.stack([q, q[::-1]])))
    assert R.same_bits(_np(got[0]), R.tri_rows(vol[0], q)) and R.same_bits(_np(got[1]), R.tri_rows(vol[1], q[::-1]))


# ------------------------------------------------------------------------------------------------ sampler: brick kernel
BRICKS = [((3, 4, 5), 5), ((6, 6, 6), 6), ((1, 4, 6), 7), ((5, 9, 3), 9), ((1, 1, 1), 2), ((2, 2, 2), 2), ((5, 7, 9), 11)]


def _lattice(vol, Q, m0, M, C, layout):
    buf, win, idx = _window(M, C, layout)
    ops.trilinear_sample(vol, Q=Q, m0=m0, M=M, out=win)
    assert _surroundings_untouched(buf, idx), (Q, m0, M, C, layout)
    return _np(win)


@pytest.mark.parametrize("C", [32, 96, 160])
@pytest.mark.parametrize("dims,Q", BRICKS, ids=lambda v: ids_dims(v) if isinstance(v, tuple) else f"Q{v}")
def test_brick_sampler(dims, Q, C):
    """whole lattices and a range of two slabs that starts on a slab that is no multiple of four (i_begin = 1): trilinear_brick_kernel"""
    vol = R.spread(dims + (C,), Q + C)
    want = R.tri_rows(vol, R.lattice_queries(Q, 0, Q ** 3))
    vd = _dev(vol)
    for layout in LAYOUTS:
        assert R.same_bits(_lattice(vd, Q, 0, Q ** 3, C, layout), want), (dims, Q, C, layout)
        if Q >= 3:
            assert R.same_bits(_lattice(vd, Q, Q * Q, 2 * Q * Q, C, layout), want[Q * Q:3 * Q * Q]), (dims, Q, C, layout, "slabs 1..2")


@pytest.mark.parametrize("dims,Q", [((3, 4, 5), 5), ((1, 4, 6), 7)], ids=lambda v: ids_dims(v) if isinstance(v, tuple) else f"Q{v}")
def test_brick_sampler_non_finite_voxels(dims, Q):
    """The brick reads a corner past an upper face as corner 0 with weight 0 instead of skipping it.  Its rule, asserted exactly: the result is NaN
    where tri_rows gives +-inf AND the query's cell corner (x0, y0, z0) holds +-inf AND the cell touches an upper face (x0 = W - 1, y0 = H - 1 or
    z0 = D - 1: the last lattice plane of an axis; every query on a size-1 axis); everywhere else it has tri_rows' bits.  Hence the two weaker
    statements: equal wherever tri_rows is finite, non-finite exactly where tri_rows is."""
    C = 32
    D, H, W = dims
    vol = _non_finite_volume(dims, C, 50 + Q)
    q = R.lattice_queries(Q, 0, Q ** 3)
    want = R.tri_rows(vol, q)
    (x0, _, _), (y0, _, _), (z0, _, _) = R.tri_axis(q[:, 0], W), R.tri_axis(q[:, 1], H), R.tri_axis(q[:, 2], D)
    face = (x0 == W - 1) | (y0 == H - 1) | (z0 == D - 1)
    turns = np.isinf(want) & np.isinf(vol[z0, y0, x0]) & face[:, None]
    assert turns.any() and np.isinf(want[~turns]).any()
    ruled = np.where(turns, np.float32(np.nan), want)
    for layout in LAYOUTS:
        got = _lattice(_dev(vol), Q, 0, Q ** 3, C, layout)
        fin = np.isfinite(want)
        assert np.array_equal(got.view(np.int32)[fin], want.view(np.int32)[fin])
        assert np.array_equal(np.isfinite(got), fin)
        assert R.same_bits(got, ruled), (dims, Q, layout)
        # the per-query kernel on the same lattice rows (a range that starts off a slab) keeps ATen's bits
        assert R.same_bits(_lattice(_dev(vol), Q, 1, Q ** 3 - 1, C, layout), want[1:])


# ------------------------------------------------------------------------------------------------ sampler: batch entry
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", [3, 24, 32])
@pytest.mark.parametrize("B,M", [(1, 1), (1, 33), (3, 1), (3, 33)])
def test_sampler_batch(B, M, C, layout):
    vol = R.spread((B,) + R.BASE_DIMS + (C,), 60 + C + B)
    q = np.stack([R.query_table(R.BASE_DIMS, n=M, seed=70 + b) for b in range(B)])
    buf, win, idx = _window(M, C, layout, lead=(B,))
    ops.trilinear_sample_batch(_dev(vol), _dev(q), out=win)
    assert _surroundings_untouched(buf, idx)
    for b in range(B):
        assert R.same_bits(_np(win[b]), R.tri_rows(vol[b], q[b])), (b, B, M, C, layout)
    if layout == "contiguous":                                          # the wrapper's own buffer (leading dimension padded to 4)
        own = ops.trilinear_sample_batch(_dev(vol), _dev(q))
        assert _bits(own, win)


# ------------------------------------------------------------------------------------------------ fp32 decoder
def _dev_layers(raw):
    dv = lambda t: None if t is None else t.contiguous().to(DEV)  # noqa: E731
    return tuple((ops.pack_kpair(w).to(DEV) if i < 2 else w.contiguous().to(DEV), b.to(DEV), dv(s), dv(t), w.shape[0]) for i, (w, b, s, t) in enumerate(raw))


@functools.lru_cache(maxsize=None)
def _case(widths, bn, M):
    raw = R.make_layers(widths, bn)
    rows = R.decoder_rows(widths[0], M)
    return raw, rows, R.decoder_fp64(rows, raw), R.decoder_fp32_bound(rows, raw)


def _decode_rows(layers, rows, OUT, layout, **kw):
    """gn_implicit_decode on pre-sampled rows, xin and out in `layout` -> out (cpu tensor)"""
    M, C0 = rows.shape
    xbuf, xin, _ = _window(M, C0, layout, a=4)
    xin.copy_(rows.to(DEV))
    obuf, out, oidx = _window(M, OUT, layout, a=1)
    ops.implicit_decode(None, layers, M=M, xin=xin, out=out, **kw)
    assert _surroundings_untouched(obuf, oidx)
    return out.cpu()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bn", list(R.BN_MODES))
@pytest.mark.parametrize("widths", R.WIDTH_SETS, ids=ids_widths)
def test_decoder_fp32_against_fp64_under_the_rounding_bound(widths, bn, layout):
    worst = 0.0
    layers = _dev_layers(R.make_layers(widths, bn))
    for M in R.ROW_COUNTS:
        raw, rows, ref, bound = _case(widths, bn, M)
        out = _decode_rows(layers, rows, widths[3], layout)
        err = (out.double() - ref).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool(torch.isfinite(out).all()) and bool((err <= bound).all()), (widths, bn, layout, M, float((err / bound).max()))
        if layout == "wide":
            assert _bits(out, _decode_rows(layers, rows, widths[3], "contiguous")), (widths, bn, M)
    print(f"[decoder-error] {ids_widths(widths)} bn={bn} {layout}: largest error / bound {worst:.3e}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("widths", [(32, 256, 256, 1), (64, 512, 256, 2)], ids=ids_widths)
def test_decoder_batch_entry_under_the_rounding_bound(widths, B):
    M, OUT = 33, widths[3]
    raw = R.make_layers(widths, "middle")
    rows = torch.stack([R.decoder_rows(widths[0], M, seed=b) for b in range(B)])
    layers = _dev_layers(raw)
    for layout in LAYOUTS:
        xbuf, xin, _ = _window(M, widths[0], layout, a=4, lead=(B,))
        xin.copy_(rows.to(DEV))
        obuf, out, oidx = _window(M, OUT, layout, a=1, lead=(B,))
        ops.implicit_decode_batch(xin, layers, out)
        assert _surroundings_untouched(obuf, oidx)
        for b in range(B):
            err = (out[b].cpu().double() - R.decoder_fp64(rows[b], raw)).abs()
            assert bool((err <= R.decoder_fp32_bound(rows[b], raw)).all()), (widths, B, b, layout)
            assert _bits(out[b], ops.implicit_decode(None, layers, M=M, xin=xin[b])), (widths, B, b, layout)


@pytest.mark.parametrize("widths", [(128, 256, 256, 3), (32, 256, 512, 4)], ids=ids_widths)
def test_decoder_is_a_pure_function_of_the_row(widths):
    raw, rows, _, _ = _case(widths, "all", 65)
    layers = _dev_layers(raw)
    one = rows[7:8]
    out = _decode_rows(layers, one.repeat(96, 1), widths[3], "contiguous")
    assert _bits(out, out[:1].repeat(96, 1))
    for pos in range(32):                                               # the same row at every position of a 32-row tile, other rows around it
        tile = rows[8:40].clone()
        tile[pos] = one[0]
        assert _bits(_decode_rows(layers, tile, widths[3], "contiguous")[pos], out[0]), pos


def _big_rows(n, c0, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = ops.new_rows(n, c0, DEV)
    x.copy_(torch.randn(n, c0, generator=g, device=DEV))
    return x


def test_decoder_grid_stride_loop():
    """M = 4096 x 32 + 33 rows: past DEC_MAX_GRID workgroups of 32 rows the kernel walks the row tiles; every row of the second pass and one in 64 of
    the first equal the same rows decoded in a call of their own, and stay inside the fp64 bound"""
    widths = (32, 256, 256, 1)
    raw = R.make_layers(widths, "all")
    layers = _dev_layers(raw)
    M = 4096 * 32 + 33
    x = _big_rows(M, 32, 1)
    out = torch.full((M, 1), NAN, device=DEV)
    ops.implicit_decode(None, layers, M=M, xin=x, out=out)
    assert bool(torch.isfinite(out).all())
    pick = torch.cat([torch.arange(0, 4096 * 32, 64), torch.arange(4096 * 32, M)]).to(DEV)
    sub = ops.new_rows(len(pick), 32, DEV)
    sub.copy_(x[pick])
    assert _bits(out[pick], ops.implicit_decode(None, layers, M=len(pick), xin=sub))
    err = (out[pick].cpu().double() - R.decoder_fp64(sub.cpu(), raw)).abs()
    bound = R.decoder_fp32_bound(sub.cpu(), raw)
    print(f"[decoder-error] grid-stride loop: largest error / bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())


def test_decoder_batch_grid_stride_loop():
    """B = 3: the cap is 4096 / 3 = 1365 workgroups per row set; M = 1365 x 32 + 33"""
    widths = (32, 256, 256, 1)
    raw = R.make_layers(widths, "all")
    layers = _dev_layers(raw)
    B, M = 3, 1365 * 32 + 33
    x = _big_rows(B * M, 32, 2).view(B, M, 32)
    out = torch.full((B, M, 1), NAN, device=DEV)
    ops.implicit_decode_batch(x, layers, out)
    assert bool(torch.isfinite(out).all())
    pick = torch.cat([torch.arange(0, 1365 * 32, 64), torch.arange(1365 * 32, M)]).to(DEV)
    for b in range(B):
        sub = ops.new_rows(len(pick), 32, DEV)
        sub.copy_(x[b][pick])
        assert _bits(out[b][pick], ops.implicit_decode(None, layers, M=len(pick), xin=sub)), b
        err = (out[b][pick].cpu().double() - R.decoder_fp64(sub.cpu(), raw)).abs()
        assert bool((err <= R.decoder_fp32_bound(sub.cpu(), raw)).all()), b


# ------------------------------------------------------------------------------------------------ the sampler inside gn_implicit_decode
@pytest.mark.parametrize("dims", [R.BASE_DIMS] + R.GEOMETRIES, ids=ids_dims)
def test_in_kernel_sampler_is_the_sampler(dims):
    """vol + query and vol + lattice through gn_implicit_decode == gn_trilinear_sample followed by gn_implicit_decode(xin), bit for bit"""
    widths = (32, 256, 256, 1)
    layers = _dev_layers(R.make_layers(widths, "all"))
    vd = _dev(R.spread(dims + (32,), 80 + sum(dims)))
    qd = _dev(R.query_table(dims, seed=32))
    for M in (len(qd), 1, 33):
        q = qd[:M].contiguous()
        want = ops.implicit_decode(None, layers, M=M, xin=ops.trilinear_sample(vd, query=q))
        got = torch.full((M, 1), NAN, device=DEV)
        ops.implicit_decode(vd, layers, query=q, out=got)
        assert _bits(got, want), (dims, M)
    Q = 7
    for m0, M in ((5, Q ** 3 - 5), (5, 1), (5, 33), (0, Q ** 3)):
        want = ops.implicit_decode(None, layers, M=M, xin=ops.trilinear_sample(vd, Q=Q, m0=m0, M=M))
        got = torch.full((M, 1), NAN, device=DEV)
        ops.implicit_decode(vd, layers, Q=Q, m0=m0, M=M, out=got)
        assert _bits(got, want), (dims, "lattice", m0, M)


def test_nan_query_component_samples_source_index_0_in_kernel_sampler():
    layers = _dev_layers(R.make_layers((32, 256, 256, 1), "all"))
    vd = _dev(R.spread(R.BASE_DIMS + (32,), 5))
    q, z = _nan_queries()
    got, want = ops.implicit_decode(vd, layers, query=_dev(q)), ops.implicit_decode(vd, layers, query=_dev(z))
    assert _bits(got, want) and bool(torch.isfinite(got).all())
    assert _bits(got, ops.implicit_decode(None, layers, M=len(q), xin=_dev(R.tri_rows(_np(vd), q))))


# ------------------------------------------------------------------------------------------------ gate
def _every_bit_left(out):
    """every element still holds the bit pattern of the NaN the buffer was filled with (not merely some NaN)"""
    prefill = torch.full((1,), NAN, dtype=torch.float32).view(torch.int32)
    return bool((out.detach().cpu().contiguous().view(torch.int32) == prefill).all())


@pytest.mark.parametrize("flag", [0.0, -0.0, 1.0])
def test_run_if_gates_the_single_call(flag):
    widths = (32, 256, 256, 3)
    raw = R.make_layers(widths, "all")
    layers, rows = _dev_layers(raw), R.decoder_rows(32, 65)
    run_if = torch.tensor([flag], device=DEV)
    out = _decode_rows(layers, rows, 3, "wide", run_if=run_if)
    if flag == 1.0:
        assert _bits(out, _decode_rows(layers, rows, 3, "wide"))
    else:
        assert _every_bit_left(out)


def test_run_if_gates_each_row_set_of_the_batch_call():
    widths = (32, 256, 256, 3)
    layers = _dev_layers(R.make_layers(widths, "all"))
    rows = torch.stack([R.decoder_rows(32, 65, seed=b) for b in range(3)]).to(DEV)
    flags = torch.tensor([[9.0, 1.0], [9.0, -0.0], [9.0, 1.0]], device=DEV)      # the flag of set b at flags[b][1]: stride 2
    out = torch.full((3, 65, 3), NAN, device=DEV)
    ops.implicit_decode_batch(rows, layers, out, run_if=flags[:, 1:], run_if_stride=flags.stride(0))
    assert _every_bit_left(out[1])
    for b in (0, 2):
        assert _bits(out[b], ops.implicit_decode(None, layers, M=65, xin=rows[b]))


# ------------------------------------------------------------------------------------------------ errors before any launch
def _plain_layers(widths, bn=(True, True, True)):
    g = torch.Generator().manual_seed(sum(widths))
    return [(torch.randn(widths[i + 1], widths[i], generator=g) * 0.1, torch.randn(widths[i + 1], generator=g) * 0.1,
             torch.rand(widths[i + 1], generator=g) + 0.5 if bn[i] else None, torch.randn(widths[i + 1], generator=g) * 0.1 if bn[i] else None) for i in range(3)]


def _refused(call, *outs):
    with pytest.raises((ValueError, TypeError)):
        call()
    torch.cuda.synchronize()
    return all(bool(torch.isnan(o).all()) for o in outs)


@pytest.mark.parametrize("case", ["C0=48", "N1=128", "OUT=0", "OUT=5", "s without t", "ldxin % 4", "ldo < OUT", "LDS", "lattice range"])
def test_decoder_refuses_before_any_launch(case):
    M = 40
    widths = {"C0=48": (48, 256, 256, 1), "N1=128": (32, 128, 256, 1), "OUT=0": (32, 256, 256, 0), "OUT=5": (32, 256, 256, 5),
              "LDS": (1024, 1024, 256, 1)}.get(case, (32, 256, 256, 3))
    raw = _plain_layers(widths)
    if case == "s without t":
        raw[1] = raw[1][:3] + (None,)
    layers = _dev_layers(raw)
    out = torch.full((M, 8), NAN, device=DEV)
    xin = torch.zeros((M, widths[0] + 2), device=DEV)
    if case == "ldxin % 4":
        assert _refused(lambda: ops.implicit_decode(None, layers, M=M, xin=xin[:, :32], out=out), out)
    elif case == "ldo < OUT":
        assert _refused(lambda: ops.implicit_decode(None, layers, M=M, xin=xin.new_zeros(M, 32), out=out.view(-1, 2)[:M]), out)
    elif case == "lattice range":
        vol = torch.zeros(R.BASE_DIMS + (32,), device=DEV)
        assert _refused(lambda: ops.implicit_decode(vol, layers, Q=4, m0=60, M=5, out=out), out)
        assert _refused(lambda: ops.implicit_decode(vol, layers, Q=1, m0=0, M=1, out=out), out)
    else:
        assert _refused(lambda: ops.implicit_decode(None, layers, M=M, xin=xin.new_zeros(M, widths[0]), out=out), out)
        out2 = torch.full((2, M, 8), NAN, device=DEV)
        assert _refused(lambda: ops.implicit_decode_batch(xin.new_zeros(2, M, widths[0]), layers, out2[:, :, :max(widths[3], 1)]), out2)


# ------------------------------------------------------------------------------------------------ wrappers and alignment
def test_wrappers_refuse_a_volume_that_is_not_packed_fp32():
    layers = _dev_layers(R.make_layers((32, 256, 256, 1), "all"))
    q = torch.rand(9, 3, device=DEV)
    vol = torch.randn(R.BASE_DIMS + (32,), device=DEV)
    views = [vol.double(), vol.permute(3, 0, 1, 2).contiguous().permute(1, 2, 3, 0), vol[:, :, ::2], vol[..., :24]]
    for v in views:
        out_s, out_d = torch.full((9, 32), NAN, device=DEV), torch.full((9, 1), NAN, device=DEV)
        assert _refused(lambda: ops.trilinear_sample(v, query=q, out=out_s[:, :v.shape[-1]]), out_s)
        assert _refused(lambda: ops.implicit_decode(v, layers, query=q, out=out_d), out_d)
    assert _refused(lambda: ops.trilinear_sample_batch(vol.double()[None], q[None]))
    assert _refused(lambda: ops.trilinear_sample_batch(views[1][None], q[None]))
    assert _refused(lambda: ops.implicit_decode(None, layers, M=9, xin=torch.zeros(9, 32, dtype=torch.float64, device=DEV)))
    # the batch wrappers: float64 operands, row sets that are not packed back to back, rows of non-unit stride
    rows, out_d = torch.zeros(2, 9, 32, device=DEV), torch.full((2, 9, 1), NAN, device=DEV)
    tall, tall_o, out_s = torch.zeros(2, 12, 32, device=DEV), torch.full((2, 12, 1), NAN, device=DEV), torch.full((2, 12, 32), NAN, device=DEV)
    assert _refused(lambda: ops.implicit_decode_batch(rows.double(), layers, out_d), out_d)
    assert _refused(lambda: ops.implicit_decode_batch(rows, layers, out_d.double()))
    assert _refused(lambda: ops.implicit_decode_batch(tall[:, :9], layers, out_d), out_d)
    assert _refused(lambda: ops.implicit_decode_batch(rows, layers, tall_o[:, :9]), tall_o)
    assert _refused(lambda: ops.implicit_decode_batch(torch.zeros(2, 32, 9, device=DEV).transpose(1, 2), layers, out_d), out_d)
    vol2, q2 = torch.stack([vol, vol]), torch.rand(2, 9, 3, device=DEV)
    assert _refused(lambda: ops.trilinear_sample_batch(vol2, q2, out=out_s[:, :9]), out_s)
    assert _refused(lambda: ops.trilinear_sample_batch(vol2, q2, out=out_s.double()[:, :9]))


@pytest.mark.parametrize("C,off", [(8, 1), (8, 2), (32, 3), (6, 1), (130, 3)])
def test_sampler_refuses_a_base_pointer_its_mode_cannot_use(C, off):
    """16-byte mode (C = 8, 32 with ldo % 4 == 0) needs 16-byte bases, the 8-byte mode (C = 6, 130) 8-byte ones: refused before any launch"""
    M, ld = 9, C + 8
    q = torch.rand(M, 3, device=DEV)
    vol = torch.randn(R.BASE_DIMS + (C,), device=DEV)
    flat = torch.zeros(vol.numel() + 8, device=DEV)
    shifted = flat[off:off + vol.numel()].view(vol.shape)              # contiguous, its base `off` floats past an aligned address
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4 * off
    buf = torch.full((M + 1, ld), NAN, device=DEV)
    out = torch.full((M, ld), NAN, device=DEV)
    assert _refused(lambda: ops.trilinear_sample(vol, query=q, out=buf[:M, off:off + C]), buf)
    assert _refused(lambda: ops.trilinear_sample(shifted, query=q, out=out[:, :C]), out)
    assert _refused(lambda: ops.trilinear_sample_batch(vol[None], q[None], out=buf[None, :M, off:off + C]), buf)
    assert _refused(lambda: ops.trilinear_sample_batch(shifted[None], q[None], out=out[None, :, :C]), out)
    ops.trilinear_sample(vol, query=q, out=out[:, :C])                  # the aligned call is served
    assert bool(torch.isfinite(out[:, :C]).all())


def test_brick_and_decoder_refuse_misaligned_rows():
    Q, C = 5, 32
    vol = torch.randn(R.BASE_DIMS + (C,), device=DEV)
    buf = torch.full((Q ** 3, C + 8), NAN, device=DEV)
    assert _refused(lambda: ops.trilinear_sample(vol, Q=Q, m0=0, M=Q ** 3, out=buf[:, 2:2 + C]), buf)      # ldo % 4 == 0, base 8 bytes off: the brick's float4
    flat = torch.zeros(vol.numel() + 4, device=DEV)
    assert _refused(lambda: ops.trilinear_sample(flat[2:2 + vol.numel()].view(vol.shape), Q=Q, m0=0, M=Q ** 3, out=buf[:, :C]), buf)
    layers = _dev_layers(R.make_layers((32, 256, 256, 1), "all"))
    out = torch.full((Q ** 3, 1), NAN, device=DEV)
    xin = torch.zeros((Q ** 3, C + 8), device=DEV)
    for off in (1, 2, 3):
        assert _refused(lambda: ops.implicit_decode(None, layers, M=Q ** 3, xin=xin[:, off:off + C], out=out), out)
        assert _refused(lambda: ops.implicit_decode_batch(xin[None, :, off:off + C], layers, out[None]), out)
    ops.implicit_decode(None, layers, M=Q ** 3, xin=xin[:, 4:4 + C], out=out)                              # row slices at 16-byte offsets stay legal
    ops.implicit_decode(None, layers, M=Q ** 3 - 3, xin=ops.new_rows(Q ** 3, C, DEV).zero_()[3:], out=out[3:])     # and row ranges of new_rows buffers
    assert bool(torch.isfinite(out).all())
