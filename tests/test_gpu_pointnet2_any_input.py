"""GPU (-m gpu): PointNet++ and the gridding at any cloud size, kNN k and torch_scatter reduction, and aggregator widths that are not multiples of 16.

Farthest-point sampling past the LDS-resident kernel's 36 864 points per example (gn_fps_nested_ws: running distances in a device workspace), kNN
interpolation for k > 8 (gn_knn_interpolate_any), the sum / add / min / mul reductions of gn_grid_scatter_ex, and whole pipelines with each of them,
against the oracle (oracle/, oracle/pipeline.py).  Where the C oracle stops (knn k <= 16, fps without a start index) a numpy restatement of its loop
is the yardstick, itself held to the oracle where both run.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from oracle import pipeline as P  # noqa: E402
from garmentnets_amd import ops, synthetic as S  # noqa: E402
from garmentnets_amd.batch import Batch  # noqa: E402
from garmentnets_amd.components.pointnet2 import Segments  # noqa: E402

DEV = "cuda:0"


def _threads():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


def _ragged_cloud(sizes, seed):
    xs, ps, bs = [], [], []
    for b, n in enumerate(sizes):
        x, p, _ = S.synthetic_cloud(1, n, seed=seed + b)
        xs.append(x); ps.append(p); bs.append(torch.full((n,), b, dtype=torch.int64))
    return torch.cat(xs), torch.cat(ps), torch.cat(bs)


def _sqd(p, q):
    """the oracle's sqdist3 in fp32: (dx*dx + dy*dy) + dz*dz"""
    d = (p - q).astype(np.float32)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _fps_np(pos, start, m):
    """gno_fps's loop for one example, begun at local point `start`: arg-max of the running distance, first maximum = lowest index"""
    pos = np.asarray(pos, np.float32)
    out = [start]
    dist = _sqd(pos, pos[start])
    for _ in range(1, m):
        last = int(np.argmax(dist))
        out.append(last)
        dist = np.minimum(dist, _sqd(pos, pos[last]))
    return np.asarray(out, np.int64)


def _fps_gpu(pos, sizes, ratio, start=None):
    seg = Segments(sizes, DEV)
    cseg = Segments([ops.fps_count(n, ratio) for n in sizes], DEV)
    idx = ops.fps(pos.to(DEV), seg.ptr, cseg.ptr, max(sizes), cseg.total, start)
    return idx.cpu().numpy().astype(np.int64), cseg


# ------------------------------------------------------------------------------------------------ farthest-point sampling
@pytest.mark.parametrize("sizes,ratio", [([36865], 0.5), ([60000, 6000, 1], 0.25), ([131072], 0.02)])
def test_fps_past_the_lds_limit_bit_exact(sizes, ratio):
    _, pos, batch = _ragged_cloud(sizes, 5)
    ref, optr = O.fps(pos.numpy(), O.batch_to_ptr(batch.numpy()), ratio)
    got, cseg = _fps_gpu(pos, sizes, ratio)
    assert list(cseg.ptr.cpu().numpy()) == list(optr)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("n", [40000, 17000])
def test_fps_large_cloud_ties_keep_the_lowest_index(n):
    """n points on a coarse integer lattice: exact ties of the running distance inside a thread, a wave and across waves; running distances in the
    workspace (40 000) and in LDS (17 000)"""
    g = torch.Generator().manual_seed(11)
    pos = torch.randint(0, 9, (n, 3), generator=g).float() * 0.125
    ref, _ = O.fps(pos.numpy(), np.array([0, n], np.int64), 0.25)
    got, _ = _fps_gpu(pos, [n], 0.25)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("sizes,starts", [([40000, 37000], [12345, 36999]), ([17000, 16385], [12345, 16384])])
def test_fps_large_cloud_start_index(sizes, starts):
    _, pos, _ = _ragged_cloud(sizes, 8)
    ratio = 0.02
    m = [ops.fps_count(n, ratio) for n in sizes]
    # the restatement is the oracle's loop: held to it from the first point
    ref0, _ = O.fps(pos[:sizes[0]].numpy(), np.array([0, sizes[0]], np.int64), ratio)
    assert np.array_equal(_fps_np(pos[:sizes[0]].numpy(), 0, m[0]), ref0)
    start = torch.tensor(starts, dtype=torch.int32, device=DEV)
    got, _ = _fps_gpu(pos, sizes, ratio, start)
    off = 0
    for b, n in enumerate(sizes):
        want = _fps_np(pos[off:off + n].numpy(), starts[b], m[b]) + off
        assert np.array_equal(got[sum(m[:b]):sum(m[:b + 1])], want), ("example", b)
        off += n


def test_fps_nested_cascade_past_the_lds_limit():
    """the SA1 -> SA2 cascade of an 80 000-point example: SA1 samples 40 000 points, so SA2 runs past the old limit too (gap_out / nested_gap)"""
    n = 80000
    _, pos, _ = _ragged_cloud([n], 13)
    pos_d = pos.to(DEV)
    seg = Segments([n], DEV)
    m1 = [ops.fps_count(n, 0.5)]
    seg1 = Segments(m1, DEV)
    gap1 = torch.empty(1, dtype=torch.float32, device=DEV)
    idx1 = ops.fps(pos_d, seg.ptr, seg1.ptr, n, seg1.total, gap_out=gap1)
    ref1, _ = O.fps(pos.numpy(), np.array([0, n], np.int64), 0.5)
    assert np.array_equal(idx1.cpu().numpy().astype(np.int64), ref1)
    assert float(gap1.cpu()[0]) > 0
    pos1 = pos_d[idx1.long()].contiguous()
    m2 = [ops.fps_count(m1[0], 0.25)]
    seg2 = Segments(m2, DEV)
    gap2 = torch.empty(1, dtype=torch.float32, device=DEV)
    plain = ops.fps(pos1, seg1.ptr, seg2.ptr, m1[0], seg2.total)
    nested = ops.fps(pos1, seg1.ptr, seg2.ptr, m1[0], seg2.total, gap_out=gap2, nested_gap=gap1)
    assert torch.equal(plain, nested)
    ref2, _ = O.fps(pos1.cpu().numpy(), np.array([0, m1[0]], np.int64), 0.25)
    assert np.array_equal(nested.cpu().numpy().astype(np.int64), ref2)
    assert np.array_equal(nested.cpu().numpy(), np.arange(m2[0]))


# ------------------------------------------------------------------------------------------------ kNN interpolation
def _knn_np(xs, ps, ptr_s, pq, ptr_q, k):
    """gno_knn_interpolate's loop for any k: neighbours in ascending (d2, index), weights and weighted sums accumulated in that order in fp32"""
    out = np.zeros((len(pq), xs.shape[1]), np.float32)
    for b in range(len(ptr_s) - 1):
        s, e = int(ptr_s[b]), int(ptr_s[b + 1])
        for q in range(int(ptr_q[b]), int(ptr_q[b + 1])):
            d = _sqd(ps[s:e], pq[q])
            order = np.lexsort((np.arange(e - s), d))[:k]
            acc = np.zeros(xs.shape[1], np.float32)
            wsum = np.float32(0)
            for t in order:
                w = np.float32(1) / np.maximum(d[t], np.float32(1e-16))
                wsum = np.float32(wsum + w)
                acc = (acc + xs[s + t] * w).astype(np.float32)
            out[q] = acc / wsum
    return out


@pytest.mark.parametrize("k", [9, 16, 33, 64])
def test_knn_interpolate_any_k(k):
    sizes = [1500, 700, 120]
    _, pos, batch = _ragged_cloud(sizes, 17)
    ptr = O.batch_to_ptr(batch.numpy())
    sidx, sptr = O.fps(pos.numpy(), ptr, 0.25)            # sources: 375, 175 and 30 points -- the last example has fewer than k = 33, 64
    xs = torch.randn(len(sidx), 70, generator=torch.Generator().manual_seed(k))
    ps = pos[torch.from_numpy(sidx)]
    out = ops.knn_interpolate(xs.to(DEV), ps.contiguous().to(DEV), Segments(list(np.diff(sptr)), DEV).ptr, pos.to(DEV),
                              Segments(sizes, DEV).ptr, k).cpu().numpy()
    if k <= 16:                                            # (the C oracle's own limit)
        ref = O.knn_interpolate(xs.numpy(), ps.numpy(), sptr, pos.numpy(), ptr, k)
        np.testing.assert_allclose(_knn_np(xs.numpy(), ps.numpy(), sptr, pos.numpy(), ptr, k), ref, rtol=1e-5, atol=1e-6)
    else:
        ref = _knn_np(xs.numpy(), ps.numpy(), sptr, pos.numpy(), ptr, k)
    np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ scatter
def _collide(N, C, B, G, seed):
    """N points over B x G^3 cells, most of them in a handful of cells (hundreds of points each), values near 1 (products stay finite)"""
    g = torch.Generator().manual_seed(seed)
    cells = B * G ** 3
    hot = torch.randint(0, cells, (5,), generator=g)
    flat = torch.where(torch.rand(N, generator=g) < 0.7, hot[torch.randint(0, 5, (N,), generator=g)], torch.randint(0, cells, (N,), generator=g))
    src = 1 + 0.01 * torch.randn(N, C, generator=g)
    return src.float(), flat.to(torch.int32), cells


def _scatter(src, flat, B, G, reduce, c_real=None):
    return ops.grid_scatter(src.to(DEV).contiguous(), flat.to(DEV), B, (G, G, G), reduce, c_real=c_real).reshape(-1, src.shape[1]).cpu()


@pytest.mark.parametrize("reduce", ["sum", "add", "min"])
def test_grid_scatter_sum_min_against_scatter_reduce(reduce):
    B, G, N, C = 2, 8, 6000, 40
    src, flat, cells = _collide(N, C, B, G, 3)
    got = _scatter(src, flat, B, G, reduce)
    red = {"sum": "sum", "add": "sum", "min": "amin"}[reduce]
    ref = torch.zeros(cells, C).scatter_reduce(0, flat.long()[:, None].expand(-1, C), src, red, include_self=False)
    if reduce == "min":
        assert torch.equal(got, ref)
    else:                                                  # fp32 of an fp64 sum against a sequential fp32 sum
        ref64 = torch.zeros(cells, C, dtype=torch.float64).index_add_(0, flat.long(), src.double())
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(got.double(), ref64, rtol=1e-6, atol=1e-6)
    assert torch.equal(got, _scatter(src, flat, B, G, reduce))


def _mul_ref(src, flat, cells, c_real):
    out = torch.ones(cells, src.shape[1])
    out[:, c_real:] = 0
    for p in range(src.shape[0]):                          # torch_scatter's CPU loop: ascending point index, from the identity 1
        out[int(flat[p])] = out[int(flat[p])] * src[p]
    return out


@pytest.mark.parametrize("C,c_real", [(32, 32), (32, 20)])
def test_grid_scatter_mul_is_the_product_in_point_order(C, c_real):
    B, G, N = 2, 8, 4000
    src, flat, cells = _collide(N, C, B, G, 4)
    src[:, c_real:] = 0                                    # channel-padded rows: zeros on the pads
    got = _scatter(src, flat, B, G, "mul", c_real)
    assert torch.equal(got, _mul_ref(src, flat, cells, c_real))
    empty = torch.ones(cells, dtype=torch.bool)
    empty[flat.long()] = False
    assert torch.all(got[empty][:, :c_real] == 1) and torch.all(got[:, c_real:] == 0)
    assert torch.equal(got, _scatter(src, flat, B, G, "mul", c_real))


# ------------------------------------------------------------------------------------------------ pipelines
def _model(hp, sd):
    from garmentnets_amd.networks.conv_implicit_wnf import ConvImplicitWNFPipeline
    m = ConvImplicitWNFPipeline(**hp)
    m.load_state_dict(sd)
    return m.to(DEV).eval().requires_grad_(False)


def _predict(model, sizes, x, pos, batch, Q):
    from garmentnets_amd.predict import predict_batch
    return predict_batch(model, Batch(sizes=list(sizes), x=x, pos=pos, batch=batch).to(DEV), volume_size=Q, auto_level=True)


def _check(res, ref_wnfs, ref_bins, TOL=1e-4):
    bins = torch.cat([torch.round(r["pred_nocs"] * 63).to(torch.int64) for r in res]).cpu()
    assert torch.equal(bins, ref_bins)
    for b, ref_wnf in enumerate(ref_wnfs):
        wnf = res[b]["wnf_volume"].cpu().numpy()
        assert float(np.abs(wnf - ref_wnf).max()) <= TOL, ("garment", b, float(np.abs(wnf - ref_wnf).max()))


def _cloud(sizes, seed):
    xs, ps, bs = [], [], []
    for b, n in enumerate(sizes):
        x, p, _ = S.synthetic_cloud(1, n, seed=seed, first=b, colour="position")
        xs.append(x); ps.append(p); bs.append(torch.full((n,), b, dtype=torch.int64))
    return torch.cat(xs), torch.cat(ps), torch.cat(bs)


def _hp(**changes):
    hp = S.default_hparams(grid=32)
    for group, kv in changes.items():
        hp[group] = dict(hp[group], **kv)
    return hp


@pytest.mark.parametrize("case", ["ragged_40000", "k16", "sum", "width100"])
def test_pipeline_against_oracle(case):
    _threads()
    sizes, Q = [3000, 3000], 64
    if case == "ragged_40000":
        hp, sizes = _hp(), [40000, 6000]
    elif case == "k16":
        hp = _hp(pointnet2_params=dict(fp2_k=16, fp1_k=16))
    elif case == "sum":
        hp = _hp(volume_agg_params=dict(reduce_method="sum"))
    else:
        hp = _hp(volume_agg_params=dict(nn_channels=[137, 137, 100]), unet3d_params=dict(in_channels=100, num_groups=4))
    sd = S.synthetic_state_dict(hp, 0, planted_nocs=True)
    x, pos, batch = _cloud(sizes, 21)
    model = _model(hp, sd)
    res = _predict(model, sizes, x, pos, batch, Q)
    with torch.no_grad():
        ref = P.predict(sd, hp, x, pos, batch, Q=Q, auto_level=True)
        vin = model.volume_agg(model.pointnet2_forward(Batch(sizes=sizes, x=x, pos=pos, batch=batch).to(DEV))["nocs_data"])
    assert tuple(vin.shape) == tuple(ref["in_feature_volume"].shape)
    assert torch.equal(vin.cpu() != 0, ref["in_feature_volume"] != 0)
    _check(res, [g["wnf_volume"] for g in ref["garments"]], ref["pointnet2_result"]["nocs_data"]["nocs_bin_idx"])


@pytest.mark.parametrize("reduce", ["min", "mul"])
def test_pipeline_min_mul_against_oracle_stages(reduce):
    """P.volume_agg knows max / mean / sum / add: the min and mul volumes are composed from its point features and cell indices (torch_scatter 2.0.8:
    empty cells 0 under min, 1 under mul), then P.unet3d and P.decode_volume"""
    _threads()
    sizes, Q = [3000, 3000], 64
    hp = _hp(volume_agg_params=dict(reduce_method=reduce))
    sd = S.synthetic_state_dict(hp, 0, planted_nocs=True)
    x, pos, batch = _cloud(sizes, 23)
    B = len(sizes)
    model = _model(hp, sd)
    res = _predict(model, sizes, x, pos, batch, Q)
    with torch.no_grad():
        p2 = P.pointnet2_forward(sd, hp, x, pos, batch)
        va = dict(hp["volume_agg_params"], reduce_method="max")
        _, inter = P.volume_agg(sd, va, p2["nocs_data"], B, return_intermediates=True)
        flat, f = inter["flat_idx"], inter["point_features"]
        C, gs = f.shape[1], tuple(va["grid_shape"])
        cells = B * int(np.prod(gs))
        if reduce == "min":
            vol = torch.zeros(cells, C).scatter_reduce(0, flat[:, None].expand(-1, C), f, "amin", include_self=False)
        else:
            vol = _mul_ref(f, flat, cells, C)
        vol = vol.reshape((B,) + gs + (C,)).permute(0, 4, 1, 2, 3).contiguous()
        out = P.unet3d(sd, hp["unet3d_params"], vol)
        ref_wnfs = [P.decode_volume(sd, out[b:b + 1], Q).numpy() for b in range(B)]
        vin = model.volume_agg(model.pointnet2_forward(Batch(sizes=sizes, x=x, pos=pos, batch=batch).to(DEV))["nocs_data"]).cpu()
    torch.testing.assert_close(vin, vol, rtol=1e-4, atol=1e-4)
    _check(res, ref_wnfs, p2["nocs_data"]["nocs_bin_idx"])
