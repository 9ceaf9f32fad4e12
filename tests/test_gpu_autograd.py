"""GPU (-m gpu): gradients of the point and grid operators (csrc/grad.hip, garmentnets_amd/autograd.py).

The yardstick for every gradient is torch autograd in fp64 on the CPU over a plain-torch restatement of the operator written here (dense masks and
one-hot matrices; F.grid_sample itself for the sampler).  Every restatement's FORWARD is first held to the existing HIP forward, so a wrong
restatement cannot pass quietly.  Index inputs (fps / ball-query / kNN results, cells) are computed once by the HIP ops and shared by both sides.

Selections (max / min) must match bit for bit, the lowest index winning a tie.  Weighted gradients must stay within
4 x (the max error of torch's own fp32 autograd of the same restatement against the fp64 one) + one fp32 ulp of the largest gradient magnitude
(tests/grad_reference.py::_check): the bound is computed at test time from the fp32-torch run, not from a constant.  The fp32-torch run is on the CPU for the single operators; for the
PointNet++ composition it is on the GPU, where that network's dense layers run (the reason and the figures are written at that test).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from garmentnets_amd import autograd as A, ops  # noqa: E402
from garmentnets_amd.components.pointnet2 import Segments  # noqa: E402
from grad_reference import _check, _first_max, _gen, r_sa_gather, r_sample, r_segment_max  # noqa: E402

DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ restatements (plain torch, any dtype, CPU)
def r_scatter(src, cell, cells, reduce):
    """src (N, C), cell (N,) -> (cells, C)"""
    mask = (cell[None, :] == torch.arange(cells, device=src.device)[:, None])                       # (cells, N)
    if reduce in ("max", "min"):
        v = src if reduce == "max" else -src
        sel = _first_max(v[None].expand(cells, -1, -1), mask[:, :, None].expand(-1, -1, src.shape[1]), 1)
        return (src[None] * sel.to(src.dtype)).sum(1)
    tot = mask.to(src.dtype) @ src
    if reduce == "mean":
        tot = tot / mask.sum(1).clamp(min=1).to(src.dtype)[:, None]
    return tot


def r_global_max(h, sizes):
    out, o = [], 0
    for n in sizes:
        hv = h[o:o + n]
        out.append((hv * _first_max(hv, torch.ones_like(hv, dtype=torch.bool), 0).to(h.dtype)).sum(0) if n else h.new_zeros(h.shape[1]))
        o += n
    return torch.stack(out)


def r_knn(x, nbr, d2, n_sources):
    """nbr / d2 (Nq, k) shared data -> the interpolation matrix (no gradient through it) @ x"""
    valid = nbr >= 0
    w = valid.to(x.dtype) / d2.to(x.dtype).clamp(min=1e-16)
    coef = w / w.sum(1, keepdim=True)
    mat = torch.zeros((nbr.shape[0], n_sources), dtype=x.dtype, device=x.device)
    mat.scatter_add_(1, nbr.clamp(min=0).long(), coef)
    return mat @ x


def _grads(fn, inputs, gout, dtype):
    """gradients of sum(fn(*inputs) * gout) with respect to the float inputs that are listed as leaves, on the CPU in dtype"""
    leaves = [t.detach().cpu().to(dtype).requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    return out.detach(), torch.autograd.grad(out, leaves, gout.detach().cpu().to(dtype))


def _hip_grads(fn, inputs, gout):
    leaves = [t.detach().to(DEV).requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    assert out.grad_fn is not None
    return out.detach(), torch.autograd.grad(out, leaves, gout.to(DEV))


# ------------------------------------------------------------------------------------------------ 1. selections: exact
def _cells_cloud(n, c, cells, seed, ties=True):
    g = _gen(seed)
    src = torch.randn(n, c, generator=g)
    cell = torch.randint(0, cells, (n,), generator=g)
    if ties:
        src[n // 2:n // 2 + n // 4] = src[:n // 4]            # duplicated rows ...
        cell[n // 2:n // 2 + n // 4] = cell[:n // 4]          # ... in the same cells: exact ties, the lower index must win
        cell[-20:] = 3
        src[-20:, 0] = 7.0                                    # a cell holding equal values (the maximum of channel 0)
        src[-20:, 1] = -7.0                                   # (the minimum of channel 1)
    return src, cell.to(torch.int32)


@pytest.mark.parametrize("reduce", ["max", "min"])
def test_grid_scatter_selection_gradient_is_exact(reduce):
    n, c, cells = 400, 8, 64
    src, cell = _cells_cloud(n, c, cells, 1)
    gout = torch.randn(cells, c, generator=_gen(2))
    fwd64, (g64,) = _grads(lambda s: r_scatter(s, cell.long(), cells, reduce), [src], gout, torch.float64)
    out, (g,) = _hip_grads(lambda s: A.scatter(s.t(), cell.to(DEV).long(), -1, cells, reduce).t(), [src], gout)
    assert torch.equal(out.cpu(), fwd64.float())                                  # the restatement's forward IS the HIP forward
    assert torch.equal(g.cpu(), g64.float())
    # the tie rule, spelled out: the first of the twenty equal points of cell 3 takes the whole gradient
    ch = 0 if reduce == "max" else 1
    assert float(g[n - 20, ch]) == float(gout[3, ch]) and float(g[n - 19:, ch].abs().max()) == 0.0
    # every (cell, channel) hands its gradient to exactly one point
    occupied = torch.zeros(cells, dtype=torch.bool)
    occupied[cell.long()] = True
    assert int((g != 0).sum()) == int(occupied.sum()) * c


def test_segment_max_gradient_is_exact():
    M, S, C = 37, 9, 70
    g = _gen(3)
    h = torch.randn(M * S, C, generator=g)
    h[1::S] = h[0::S]                                          # slot 1 repeats slot 0: ties
    h = torch.relu(h)                                          # and many exact zeros, as behind a ReLU
    slot = torch.randint(-1, 50, (M * S,), generator=g).to(torch.int32)
    slot[5 * S:6 * S] = -1                                     # a centre with no valid slot: output 0, no gradient
    gout = torch.randn(M, C, generator=g)
    fwd64, (g64,) = _grads(lambda t: r_segment_max(t, slot, M, S), [h], gout, torch.float64)
    out, (gh,) = _hip_grads(lambda t: A._SegmentMax.apply(t, slot.to(DEV), M, S), [h], gout)
    assert torch.equal(out.cpu(), fwd64.float())
    assert torch.equal(gh.cpu(), g64.float())
    assert float(gh[5 * S:6 * S].abs().max()) == 0.0


def test_global_max_pool_gradient_is_exact():
    sizes, C = [300, 1, 0, 77], 130
    g = _gen(4)
    n = sum(sizes)
    h = torch.relu(torch.randn(n, C, generator=g))
    h[0] = h[250] = h[:300].max(0).values                     # two rows hold the maximum of every channel: row 0, the lower index, wins
    gout = torch.randn(len(sizes), C, generator=g)
    fwd64, (g64,) = _grads(lambda t: r_global_max(t, sizes), [h], gout, torch.float64)
    seg = Segments(sizes, DEV)
    out, (gh,) = _hip_grads(lambda t: A.global_max_pool(t, seg), [h], gout)
    assert torch.equal(out.cpu(), fwd64.float())
    assert torch.equal(gh.cpu(), g64.float())
    assert torch.equal(gh[0].cpu(), gout[0]) and float(gh[250].abs().max()) == 0.0


def test_first_maximum_of_the_restatement_is_the_lowest_index():
    v = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0], [5.0, 5.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    sel = _first_max(v, torch.ones_like(v, dtype=torch.bool), 1)
    assert sel.tolist() == [[False, True, False, False, False], [True, False, False, False, False]]


# ------------------------------------------------------------------------------------------------ 2. weighted gradients
@pytest.mark.parametrize("reduce", ["mean", "sum", "add"])
def test_grid_scatter_weighted_gradient(reduce):
    n, c, cells = 600, 19, 4 * 4 * 4 * 2                       # ~5 points per cell on average, some cells empty
    src, cell = _cells_cloud(n, c, cells, 5)
    cell[:200] = 9                                             # many points in one cell
    cell[cell == 11] = 12                                      # an empty cell for certain
    gout = torch.randn(cells, c, generator=_gen(6))
    fn = lambda s: r_scatter(s, cell.long(), cells, reduce)    # noqa: E731
    fwd64, (g64,) = _grads(fn, [src], gout, torch.float64)
    _, (g32,) = _grads(fn, [src], gout, torch.float32)
    out, (g,) = _hip_grads(lambda s: A.scatter(s.t(), cell.to(DEV).long(), -1, cells, reduce).t(), [src], gout)
    assert torch.allclose(out.cpu().double(), fwd64, rtol=1e-5, atol=1e-6)
    _check(f"grid_scatter[{reduce}]", g64, g32, g)


def _sa_case(seed, sizes=(300, 212), ratio=0.25, r=0.25, K=16):
    g = _gen(seed)
    n = sum(sizes)
    pos = torch.rand(n, 3, generator=g)
    seg = Segments(list(sizes), DEV)
    idx = A.fps(pos.to(DEV), seg, ratio)
    cseg = Segments([ops.fps_count(s, ratio) for s in sizes], DEV)
    nbr, _ = A.ball_table(pos.to(DEV), idx, r, seg, cseg, K)
    return pos, seg, cseg, idx, nbr


@pytest.mark.parametrize("scope", ["batch", "example"])
def test_sa_gather_gradient(scope):
    pos, seg, cseg, idx, nbr = _sa_case(7)
    C = 21
    x = torch.randn(pos.shape[0], C, generator=_gen(8))
    self_src = None
    if scope == "example":
        from garmentnets_amd.components.pointnet2 import _example_self_src
        self_src = _example_self_src(seg.sizes, cseg.sizes, DEV)
    S = nbr.shape[1] + 1
    gout = torch.randn(nbr.shape[0] * S, C + 3, generator=_gen(9))
    slot = {}

    def hip(t):
        edges, slot["s"] = A._SaGather.apply(t, pos.to(DEV), idx.to(torch.int32), nbr, True, self_src)
        return edges
    out, (g,) = _hip_grads(hip, [x], gout)
    s = slot["s"].cpu()
    fn = lambda t: r_sa_gather(t, pos.to(t.dtype), idx.cpu(), s, S)     # noqa: E731
    fwd64, (g64,) = _grads(fn, [x], gout, torch.float64)
    _, (g32,) = _grads(fn, [x], gout, torch.float32)
    assert torch.allclose(out.cpu().double(), fwd64, rtol=0, atol=1e-6)
    assert torch.equal(out[:, :C].cpu(), fwd64[:, :C].float())
    _check(f"sa_gather[{scope}]", g64, g32, g)
    # the same bits again: the sum per source point is ordered
    _, (g2,) = _hip_grads(hip, [x], gout)
    assert torch.equal(g, g2)


@pytest.mark.parametrize("k", [1, 3, 12])
def test_knn_interpolate_gradient(k):
    g = _gen(10 + k)
    src_sizes, q_sizes = [40, 7, 90], [200, 50, 333]           # the second example has fewer sources than k = 12
    ps, pq = torch.rand(sum(src_sizes), 3, generator=g), torch.rand(sum(q_sizes), 3, generator=g)
    pq[:10] = ps[:10]                                          # queries ON a source: d2 = 0, the 1e-16 clamp
    C = 45
    x = torch.randn(sum(src_sizes), C, generator=g)
    gout = torch.randn(sum(q_sizes), C, generator=g)
    sseg, qseg = Segments(src_sizes, DEV), Segments(q_sizes, DEV)
    nbr, d2 = ops.knn_neighbours(ps.to(DEV), sseg.ptr, pq.to(DEV), qseg.ptr, k)
    nbr, d2 = nbr.cpu(), d2.cpu()
    assert int((nbr[200:250] >= 0).sum(1).max()) == min(k, 7)
    fn = lambda t: r_knn(t, nbr, d2, x.shape[0])               # noqa: E731
    fwd64, (g64,) = _grads(fn, [x], gout, torch.float64)
    _, (g32,) = _grads(fn, [x], gout, torch.float32)
    hip = lambda t: A.knn_interpolate(t, ps.to(DEV), pq.to(DEV), sseg, qseg, k)     # noqa: E731
    out, (gx,) = _hip_grads(hip, [x], gout)
    assert torch.allclose(out.cpu().double(), fwd64, rtol=1e-5, atol=1e-5)
    _check(f"knn_interpolate[k={k}]", g64, g32, gx)
    _, (gx2,) = _hip_grads(hip, [x], gout)
    assert torch.equal(gx, gx2)


def _sampler_case(seed, B=3, C=20, dims=(5, 9, 3), M=500):
    """sizes - 1 are powers of two: a lattice query i / (size - 1) lands on its voxel exactly in fp32 and in fp64 alike"""
    g = _gen(seed)
    vol = torch.randn(B, C, *dims, generator=g)
    q = torch.rand(B, M, 3, generator=g)
    D, H, W = dims
    lat = torch.stack((torch.randint(0, W, (M // 4,), generator=g) / (W - 1), torch.randint(0, H, (M // 4,), generator=g) / (H - 1),
                       torch.randint(0, D, (M // 4,), generator=g) / (D - 1)), 1)
    q[:, :M // 4] = lat                                        # exactly on lattice points (the border ones included)
    q[:, M // 4:M // 2] = q[:, M // 4:M // 2] * 3.0 - 1.0      # many outside [0, 1] on one or more axes: clamped coordinates
    return vol, q


def test_trilinear_sample_gradient_both_outputs():
    vol, q = _sampler_case(20)
    gout = torch.randn(q.shape[0], q.shape[1], vol.shape[1], generator=_gen(21))
    fwd64, (gv64, gq64) = _grads(r_sample, [vol, q], gout, torch.float64)
    _, (gv32, gq32) = _grads(r_sample, [vol, q], gout, torch.float32)
    out, (gv, gq) = _hip_grads(A.grid_sample_points, [vol, q], gout)
    assert torch.allclose(out.cpu().double(), fwd64, rtol=1e-5, atol=1e-5)
    _check("trilinear_sample grad_vol", gv64, gv32, gv)
    _check("trilinear_sample grad_query", gq64, gq32, gq)
    # a coordinate clamped at the border gets gradient 0 (F.grid_sample's rule), on that axis only
    outside = ((q <= 0) | (q >= 1)).to(DEV)
    assert bool(outside.any()) and float(gq[outside].abs().max()) == 0.0
    assert float(gq[~outside].abs().max()) > 0.0
    # ordered sum per voxel: the same bits again
    _, (gv2, gq2) = _hip_grads(A.grid_sample_points, [vol, q], gout)
    assert torch.equal(gv, gv2) and torch.equal(gq, gq2)


def test_trilinear_sample_gradient_only_what_is_asked_for():
    vol, q = _sampler_case(22, B=2, C=128, dims=(9, 5, 9), M=300)
    gout = torch.randn(2, 300, 128, generator=_gen(23))
    _, (gv64, gq64) = _grads(r_sample, [vol, q], gout, torch.float64)
    _, (gv32, gq32) = _grads(r_sample, [vol, q], gout, torch.float32)
    vd, qd = vol.to(DEV).requires_grad_(True), q.to(DEV)
    (gv,) = torch.autograd.grad(A.grid_sample_points(vd, qd), [vd], gout.to(DEV))
    _check("trilinear_sample grad_vol only (C=128)", gv64, gv32, gv)
    vd, qd = vol.to(DEV), q.to(DEV).requires_grad_(True)
    (gq,) = torch.autograd.grad(A.grid_sample_points(vd, qd), [qd], gout.to(DEV))
    _check("trilinear_sample grad_query only (C=128)", gq64, gq32, gq)


# ------------------------------------------------------------------------------------------------ 4. edge cases
def test_grid_scatter_bwd_channel_padded_rows_and_repeats():
    n, c_real, C, cells = 300, 13, 16, 27
    src, cell = _cells_cloud(n, C, cells, 30)
    src[:, c_real:] = 0
    gout = torch.randn(cells, C, generator=_gen(31))
    for reduce in ("max", "min", "mean", "sum"):
        vol = ops.grid_scatter(src.to(DEV), cell.to(DEV), 1, (cells,), reduce, c_real=c_real)
        a = ops.grid_scatter_bwd(gout.to(DEV).view(vol.shape), cell.to(DEV), n, reduce, vol=vol, src=src.to(DEV), c_real=c_real)
        b = ops.grid_scatter_bwd(gout.to(DEV).view(vol.shape), cell.to(DEV), n, reduce, vol=vol, src=src.to(DEV), c_real=c_real)
        assert torch.equal(a, b), reduce
        assert float(a[:, c_real:].abs().max()) == 0.0, reduce
        _, (g64,) = _grads(lambda s: r_scatter(s, cell.long(), cells, reduce), [src], gout, torch.float64)
        if reduce in ("max", "min"):
            assert torch.equal(a[:, :c_real].cpu(), g64[:, :c_real].float()), reduce
        else:
            _, (g32,) = _grads(lambda s: r_scatter(s, cell.long(), cells, reduce), [src], gout, torch.float32)
            _check(f"grid_scatter padded[{reduce}]", g64[:, :c_real], g32[:, :c_real], a[:, :c_real])


def test_empty_inputs_give_empty_or_zero_gradients():
    vol = torch.randn(2, 4, 3, 3, 3, device=DEV, requires_grad=True)
    q = torch.rand(2, 0, 3, device=DEV, requires_grad=True)
    out = A.grid_sample_points(vol, q)
    assert out.shape == (2, 0, 4)
    gv, gq = torch.autograd.grad(out.sum(), [vol, q])
    assert gq.shape == (2, 0, 3) and float(gv.abs().max()) == 0.0
    # no queries: every source's gradient is zero
    x = torch.randn(10, 5, device=DEV, requires_grad=True)
    y = A.knn_interpolate(x, torch.rand(10, 3, device=DEV), torch.rand(0, 3, device=DEV), Segments([10], DEV), Segments([0], DEV), 3)
    (gx,) = torch.autograd.grad(y.sum(), [x])
    assert y.shape == (0, 5) and gx.shape == (10, 5) and float(gx.abs().max()) == 0.0
    # no points: an empty gradient
    assert ops.grid_scatter_bwd(torch.zeros(1, 8, 4, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), 0, "mean").shape == (0, 4)


def test_mul_is_refused_by_name():
    src = torch.rand(4, 50, device=DEV, requires_grad=True)
    idx = torch.randint(0, 8, (50,), device=DEV)
    with pytest.raises(ValueError, match="mul"):
        A.scatter(src, idx, -1, 8, "mul")
    with torch.no_grad():
        assert A.scatter(src, idx, -1, 8, "mul").shape == (4, 8)      # forward-only still runs


# ------------------------------------------------------------------------------------------------ 6. no-grad path
def test_no_grad_path_returns_the_existing_ops_bits():
    pos, seg, cseg, idx, nbr = _sa_case(40)
    n = pos.shape[0]
    x = torch.randn(n, 16, generator=_gen(41)).to(DEV)
    pd = pos.to(DEV)
    nn_ = torch.nn.Sequential(torch.nn.Linear(19, 32), torch.nn.ReLU()).to(DEV)
    vol = torch.randn(2, 8, 4, 4, 4, generator=_gen(42)).to(DEV)
    q = torch.rand(2, 50, 3, generator=_gen(43)).to(DEV)
    cell = torch.randint(0, 64, (n,), generator=_gen(44)).to(DEV)

    def run():
        return (A.point_conv_max(x, pd, idx, nbr, nn_), A.global_max_pool(x, seg),
                A.knn_interpolate(x[idx], pd[idx].contiguous(), pd, cseg, seg, 3), A.scatter(x.t(), cell, -1, 64, "mean"),
                A.scatter(x.t(), cell, -1, 64, "max"), A.grid_sample_points(vol, q))
    with torch.no_grad():
        edges, slot, S = ops.sa_gather(x, pd, idx.to(torch.int32), nbr)
        want = (ops.segment_max(nn_(edges), slot, nbr.shape[0], S), ops.global_max_pool(x, seg.ptr, seg.num),
                ops.knn_interpolate(x[idx].contiguous(), pd[idx].contiguous(), cseg.ptr, pd, seg.ptr, 3),
                ops.grid_scatter(x, cell.to(torch.int32), 1, (64,), "mean").view(64, 16).t(),
                ops.grid_scatter(x, cell.to(torch.int32), 1, (64,), "max").view(64, 16).t(),
                ops.trilinear_sample_batch(vol.permute(0, 2, 3, 4, 1).contiguous(), q))
        got = run()
    for g, w in zip(got, want):
        assert g.grad_fn is None and not g.requires_grad and torch.equal(g, w)
    for p in nn_.parameters():
        p.requires_grad_(False)
    for g, w in zip(run(), want):                               # grad mode on, but nothing requires grad
        assert g.grad_fn is None and not g.requires_grad and torch.equal(g, w)


# ------------------------------------------------------------------------------------------------ 5. composition
def _mlp(dims, gen):
    layers = []
    for a, b in zip(dims[:-1], dims[1:]):
        bn = torch.nn.BatchNorm1d(b)
        bn.weight.data = 0.5 + torch.rand(b, generator=gen)
        bn.bias.data = 0.2 * torch.randn(b, generator=gen)
        bn.running_mean.data = 0.2 * torch.randn(b, generator=gen)
        bn.running_var.data = 0.5 + torch.rand(b, generator=gen)
        layers.append(torch.nn.Sequential(torch.nn.Linear(a, b), torch.nn.ReLU(), bn))
    return torch.nn.Sequential(*layers)


class _Net(torch.nn.Module):
    """SA -> SA -> global SA -> FP x3 -> linear head, the operators handed in (HIP autograd bindings or the restatements)"""

    def __init__(self, gen, bins=8):
        super().__init__()
        self.sa1, self.sa2, self.sa3 = _mlp([3 + 3, 16, 16, 32], gen), _mlp([32 + 3, 32, 32, 64], gen), _mlp([64 + 3, 64, 128], gen)
        self.fp3, self.fp2, self.fp1 = _mlp([128 + 64, 64], gen), _mlp([64 + 32, 32], gen), _mlp([32 + 3, 32], gen)
        self.head = torch.nn.Linear(32, 3 * bins)
        self.bins = bins

    def forward(self, x, pos, op):
        x1 = op.conv(1, x, self.sa1)
        x2 = op.conv(2, x1, self.sa2)
        pos2 = pos[op.idx1.long()][op.idx2.long()]
        x3 = op.gmax(self.sa3(torch.cat((x2, pos2), 1)))
        y2 = self.fp3(torch.cat((op.interp(3, x3), x2), 1))
        y1 = self.fp2(torch.cat((op.interp(2, y2), x1), 1))
        y0 = self.fp1(torch.cat((op.interp(1, y1), x), 1))
        return self.head(y0).view(-1, 3, self.bins)


def test_pointnet2_composition_parameter_gradients():
    torch.manual_seed(0)
    sizes = [512, 512]
    g = _gen(50)
    n = sum(sizes)
    pos, x = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    target = torch.randint(0, 8, (n, 3), generator=g)
    pd = pos.to(DEV)
    seg0 = Segments(sizes, DEV)
    # the shared indices, computed once by the HIP ops
    idx1 = A.fps(pd, seg0, 0.5)
    seg1 = Segments([ops.fps_count(s, 0.5) for s in sizes], DEV)
    nbr1, _ = A.ball_table(pd, idx1, 0.2, seg0, seg1, 32)
    pos1 = pd[idx1].contiguous()
    idx2 = A.fps(pos1, seg1, 0.25)
    seg2 = Segments([ops.fps_count(s, 0.25) for s in seg1.sizes], DEV)
    nbr2, _ = A.ball_table(pos1, idx2, 0.4, seg1, seg2, 32)
    pos2 = pos1[idx2].contiguous()
    seg3 = Segments([1] * len(sizes), DEV)
    pos3 = torch.zeros(len(sizes), 3, device=DEV)
    levels = {1: (pd, idx1, nbr1), 2: (pos1, idx2, nbr2)}
    knn = {3: (pos3, seg3, pos2, seg2, 1), 2: (pos2, seg2, pos1, seg1, 3), 1: (pos1, seg1, pd, seg0, 3)}

    class Hip:
        def conv(self, lvl, xin, nn_):
            p, idx, nbr = levels[lvl]
            return A.point_conv_max(xin, p, idx, nbr, nn_)

        def gmax(self, h):
            return A.global_max_pool(h, seg2)

        def interp(self, lvl, xin):
            ps, ss, pq, sq, k = knn[lvl]
            return A.knn_interpolate(xin, ps, pq, ss, sq, k)
    Hip.idx1, Hip.idx2 = idx1, idx2

    slots = {lvl: ops.sa_gather(None, p, idx.to(torch.int32), nbr)[1].cpu() for lvl, (p, idx, nbr) in levels.items()}
    nbrs = {lvl: tuple(t.cpu() for t in ops.knn_neighbours(ps, ss.ptr, pq, sq.ptr, k)) for lvl, (ps, ss, pq, sq, k) in knn.items()}

    class Restated:
        def __init__(self, dtype, device="cpu"):
            self.dtype, self.device = dtype, device
            self.idx1, self.idx2 = idx1.to(device), idx2.to(device)

        def conv(self, lvl, xin, nn_):
            p, idx, nbr = levels[lvl]
            S = nbr.shape[1] + 1
            slot = slots[lvl].to(self.device)
            return r_segment_max(nn_(r_sa_gather(xin, p.to(self.device, self.dtype), idx.to(self.device), slot, S)), slot, nbr.shape[0], S)

        def gmax(self, h):
            return r_global_max(h, seg2.sizes)

        def interp(self, lvl, xin):
            return r_knn(xin, nbrs[lvl][0].to(self.device), nbrs[lvl][1].to(self.device), xin.shape[0])

    def param_grads(net, xin, pin, op, tgt):
        logits = net(xin, pin, op)
        loss = F.cross_entropy(logits.permute(0, 2, 1), tgt)
        return float(loss.detach()), torch.autograd.grad(loss, list(net.parameters()))

    net = _Net(_gen(51)).eval()
    state = {k: v.clone() for k, v in net.state_dict().items()}

    def fresh(dtype, device):
        m = _Net(_gen(51)).eval()
        m.load_state_dict(state)
        return m.to(device=device, dtype=dtype)
    l64, g64 = param_grads(fresh(torch.float64, "cpu"), x.double(), pos.double(), Restated(torch.float64), target)
    l32, g32 = param_grads(fresh(torch.float32, "cpu"), x, pos, Restated(torch.float32), target)
    lh, gh = param_grads(fresh(torch.float32, DEV), x.to(DEV), pd, Hip(), target.to(DEV))
    print(f"[grad-error] pointnet2 composition: loss fp64 {l64:.9f}  torch-fp32 {l32:.9f}  hip {lh:.9f}")
    assert abs(lh - l64) <= 1e-5 * abs(l64)                     # a forward sanity check (fp32 against fp64); the gradients carry the measured bound
    # torch's own fp32 autograd of the same restatement, for the bound: run ON THE GPU, where the network under test runs.  Every Linear / BatchNorm /
    # cross-entropy of the network under test is torch's GPU kernel, so "torch's own fp32 error" has to hold those same kernels and none of
    # csrc/grad.hip; the CPU's fp32 GEMMs sum in another order and are printed next to it for the record (measured on an MI355X: with the CPU run as
    # the measure, sa2.0.0.weight and sa2.1.0.weight miss by 1.2x / 1.04x -- 2.02e-10 against 1.70e-10, 6.74e-10 against 6.47e-10 -- and the GPU run
    # WITHOUT any HIP gradient kernel shows the same 2.16e-10 / 6.74e-10: the excess is the dense layers' rounding, not the operators').
    _, g32d = param_grads(fresh(torch.float32, DEV), x.to(DEV), pd, Restated(torch.float32, DEV), target.to(DEV))
    names = [k for k, _ in net.named_parameters()]
    failed = []
    for name, a, b, d, c in zip(names, g64, g32, g32d, gh):
        print(f"[grad-error] pointnet2 {name}: torch-fp32 on the CPU (for the record) {float((b.double() - a).abs().max()):.3e}")
        try:
            _check(f"pointnet2 {name}", a, d, c)
        except AssertionError as e:
            failed.append(str(e.args[0])[:200])
    assert not failed, failed


def test_second_stage_front_gradient():
    """scatter(mean) of per-point features into a 16^3 grid -> grid_sample_points at random queries -> MSE: gradient to the per-point features"""
    g = _gen(60)
    B, n, C, G, M = 2, 700, 12, 16, 400
    feat = torch.randn(B * n, C, generator=g)
    cell = torch.randint(0, G, (B * n, 3), generator=g)
    cell[:300] = cell[0]                                        # many points in one cell
    batch = torch.arange(B).repeat_interleave(n)
    flat = ((batch * G + cell[:, 0]) * G + cell[:, 1]) * G + cell[:, 2]
    q = torch.rand(B, M, 3, generator=g) * 1.2 - 0.1
    tgt = torch.randn(B, M, C, generator=g)

    def restated(f):
        vol = r_scatter(f, flat, B * G ** 3, "mean").view(B, G, G, G, C).permute(0, 4, 1, 2, 3)
        return F.mse_loss(r_sample(vol, q.to(f.dtype)), tgt.to(f.dtype))

    def hip(f):
        vol = A.scatter(f.t(), flat.to(DEV), -1, B * G ** 3, "mean").view(C, B, G, G, G).permute(1, 0, 2, 3, 4)
        return F.mse_loss(A.grid_sample_points(vol.contiguous(), q.to(DEV)), tgt.to(DEV))
    one = torch.ones(())
    l64, (g64,) = _grads(restated, [feat], one, torch.float64)
    l32, (g32,) = _grads(restated, [feat], one, torch.float32)
    lh, (gh,) = _hip_grads(hip, [feat], one)
    assert abs(float(lh) - float(l64)) <= 1e-5 * abs(float(l64))
    _check("second stage front", g64, g32, gh)
    _, (gh2,) = _hip_grads(hip, [feat], one)
    assert torch.equal(gh, gh2)
