"""CPU: the restatements of tests/decoder_reference.py are what they claim to be -- the float32 sampler is torch's grid_sample on the CPU bit for bit
on the GPU suite's geometries and queries, the lattice is the oracle's, the corner order is visible in the bits, the brick kernel's voxel box fits its
LDS allotment under the host's dispatch, and the decoder's error bound is neither broken by an honest float32 evaluation nor blind to a 1 % change
of one weight."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decoder_reference as R
from oracle import pipeline as P


def _grid_sample(vol, query):
    """vol [D][H][W][C], query [M][3] in [0, 1] -> [M][C], as ImplicitWNFDecoder.forward calls it"""
    v = torch.from_numpy(np.ascontiguousarray(vol)).permute(3, 0, 1, 2)[None]
    q = torch.from_numpy(query)
    out = F.grid_sample(v, (2.0 * q - 1.0).view(1, -1, 1, 1, 3), mode="bilinear", padding_mode="border", align_corners=True)
    return out.view(vol.shape[3], -1).t().contiguous().numpy()


@pytest.mark.parametrize("dims", [R.BASE_DIMS] + R.GEOMETRIES, ids=lambda d: "x".join(map(str, d)))
def test_tri_rows_is_grid_sample_bit_for_bit(dims):
    for C in R.GEOMETRY_CHANNELS:
        vol = R.spread(dims + (C,), 11 + C)
        q = R.query_table(dims, seed=C)
        assert not np.isnan(q).any()                                    # (NaN queries follow the project's rule, not torch's: not compared)
        assert R.same_bits(R.tri_rows(vol, q), _grid_sample(vol, q)), (dims, C)


def test_query_table_holds_what_the_gpu_tests_count_on():
    for dims in [R.BASE_DIMS] + R.GEOMETRIES:
        q = R.query_table(dims)
        assert q.shape == (R.N_QUERIES, 3) and q.dtype == np.float32
        for a, size in enumerate(dims[::-1]):
            col = q[:, a]
            assert set(R.axis_table(size).view(np.int32)) == set(col.view(np.int32))            # every table entry, signed zero included
            for k in range(size if size > 1 else 0):
                v = np.float32(k) / np.float32(size - 1)
                assert (col == v).any() and (col == np.nextafter(v, np.float32(2))).any() and (col == np.nextafter(v, np.float32(-2))).any()
            assert np.isposinf(col).any() and np.isneginf(col).any() and (col == np.float32(1e30)).any() and (col == np.float32(-0.05)).any()


def test_nan_query_component_maps_to_source_index_0():
    vol = R.spread((3, 4, 5, 3), 5)
    q = np.array([[np.nan, 0.5, 0.5], [0.5, np.nan, 0.5], [0.5, 0.5, np.nan], [np.nan] * 3], np.float32)
    z = np.where(np.isnan(q), np.float32(0), q)
    got = R.tri_rows(vol, q)
    assert not np.isnan(got).any() and R.same_bits(got, R.tri_rows(vol, z))


@pytest.mark.parametrize("Q", [2, 3, 5, 9, 32, 129])
def test_lattice_queries_are_the_oracles_grid_points(Q):
    want = P.grid_points(Q).reshape(-1, 3).numpy()
    assert R.same_bits(R.lattice_queries(Q, 0, Q ** 3), want)
    assert R.same_bits(R.lattice_queries(Q, 5, Q ** 3 - 5), want[5:])
    assert np.array_equal(np.signbit(R.lattice_queries(Q, 0, 1)), np.signbit(want[:1]))


def test_reverse_corner_order_gives_other_bits():
    """on every geometry of the suite with at least three corners inside the volume (two non-unit axes: a two-term sum commutes) and at every channel count"""
    for dims in [R.BASE_DIMS] + R.GEOMETRIES:
        for C in R.GEOMETRY_CHANNELS:
            vol, q = R.spread(dims + (C,), 11 + C), R.query_table(dims, seed=C)
            fwd, rev = R.tri_rows(vol, q), R.tri_rows(vol, q, reverse=True)
            if sum(d > 1 for d in dims) >= 2:
                assert not R.same_bits(fwd, rev), (dims, C)
            else:
                assert R.same_bits(fwd, rev), (dims, C)
    for Q, dims in ((5, (3, 4, 5)), (11, (5, 7, 9))):                   # the lattice inputs of the brick tests
        vol, q = R.spread(dims + (32,), Q), R.lattice_queries(Q, 0, Q ** 3)
        assert not R.same_bits(R.tri_rows(vol, q), R.tri_rows(vol, q, reverse=True))


def test_brick_voxel_box_fits_six_voxels_per_axis():
    """trilinear_brick_kernel stages (4 + 2)^3 voxels at most.  gn_trilinear_sample launches it for Q >= size only and a brick may start on ANY slab
    (m0 is a multiple of Q^2, not of 4 Q^2): every Q in 2 .. 256, 512 and 1024, every size <= Q, every start -- in the kernel's own fp32 coordinates"""
    worst = (0, None)
    for Q in list(range(2, 257)) + [512, 1024]:
        size, i0 = np.meshgrid(np.arange(1, Q + 1), np.arange(Q), indexing="ij")
        ext = R.brick_extent(Q, size, i0)
        assert ext.min() >= 1
        m = int(ext.max())
        if m > worst[0]:
            at = np.unravel_index(int(ext.argmax()), ext.shape)
            worst = (m, (Q, int(size[at]), int(i0[at])))
    print(f"largest brick extent {worst[0]} voxels, first at (Q, size, start) = {worst[1]}")
    assert worst[0] <= 6


@pytest.mark.parametrize("bn", list(R.BN_MODES))
@pytest.mark.parametrize("widths", R.WIDTH_SETS, ids=lambda w: "-".join(map(str, w)))
def test_decoder_bound_holds_for_torch_fp32_and_sees_a_one_percent_weight_change(widths, bn):
    """The bound is a worst case over summation orders and signs: about K u per layer relative to sum |w| |x|, 1e-3 .. 1e-1 of |y| on the dense rows,
    where an honest float32 evaluation uses a few 1e-3 of it at most (printed).  1 % of one first-layer weight among K x 256 moves a dense row's output
    by some 1e-5 of |y|, far less than the bound: no worst-case bound can see it there.  It sees it on the one-hot row (decoder_rows row 5), whose
    channel four units read: 1 % of one of their weights is 1 % of a quarter of the signal, several times the bound in every width set."""
    raw = R.make_layers(widths, bn)
    rows = R.decoder_rows(widths[0], 65)
    pre1 = rows[2].double() @ raw[0][0].double().t() + raw[0][1].double()
    assert float(pre1.max()) < 0 and not bool(rows[1].any())          # the rows the GPU suite counts on
    assert int((rows[5] != 0).sum()) == 1 and sorted(torch.nonzero(raw[0][0][:, 1]).flatten().tolist()) == R.SPARSE_UNITS
    ref, bound = R.decoder_fp64(rows, raw), R.decoder_fp32_bound(rows, raw)
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
    assert bool((ref[:, 0] > 0).all())                                  # output 0 is alive on every row
    err = (R.decoder_fp32_cpu(rows, raw).double() - ref).abs()
    print(f"{widths} bn={bn}: torch fp32 error / bound, largest {float((err / bound).max()):.2e}; bound / |y| on output 0, largest {float((bound / ref.abs())[:, 0].max()):.2e}")
    assert bool((err <= bound).all())
    w1 = raw[0][0].clone()
    w1[R.SPARSE_UNITS[0], 1] *= 1.01                                    # one weight of the first layer's 256 (or 512) x C0
    bent = [(w1,) + raw[0][1:]] + raw[1:]
    err = (R.decoder_fp32_cpu(rows, bent).double() - ref).abs()
    print(f"    1 % of w1[{R.SPARSE_UNITS[0]}][1]: error / bound, largest {float((err / bound).max()):.2f} (row {int((err / bound).max(dim=1).values.argmax())})")
    assert bool((err > bound).any())
