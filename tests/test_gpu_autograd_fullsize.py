"""GPU (-m gpu): the point and grid gradient kernels (csrc/grad.hip) ONCE at the shapes DESIGN.md times ("Operator gradients", kernel times): the
reference's validation shape, 8 x 6000 points and 24 x 6000 queries into a 32^3 x 128 volume.  The slow cases of tests/test_gpu_autograd_edges.py,
kept apart as tests/test_gpu_fullsize.py keeps the forward's: the fp64 side runs on the CPU over the sparse restatements of
tests/test_autograd_host.py (memory linear in the input; the dense ones would need cells x N masks of 10^10 entries).

Selections are bit-exact, weighted gradients follow tests/test_gpu_autograd.py's rule (4 x torch-fp32's own error + 1 ulp, measured here), and
every gradient is computed twice and must repeat bit for bit.  Each test prints its CPU-side time as `[cpu-time] ...`; the figures measured on the
MI355X host are in the tests' docstrings.
"""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import ops  # noqa: E402
from garmentnets_amd.components.pointnet2 import Segments  # noqa: E402
from test_autograd_host import s_global_max, s_knn, s_sa_gather, s_scatter, s_segment_max  # noqa: E402
from grad_reference import _check, _gen, r_sample  # noqa: E402
from test_gpu_autograd import DEV, _grads  # noqa: E402


class _CpuClock:
    def __init__(self, name):
        self.name, self.t = name, 0.0

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        self.t += time.perf_counter() - self.t0
        print(f"[cpu-time] {self.name}: {self.t:.1f} s on the CPU so far")


@pytest.mark.parametrize("reduce", ["max", "mean"])
def test_grid_scatter_bwd_at_48000_points_137_channels_8x32cubed_cells(reduce):
    """CPU side (fp64, and fp32 for mean): 1.4 s for max, 0.3 s for mean (measured on the MI355X host; the whole test 1.7 s / 0.6 s)"""
    N, C, cells = 48000, 137, 8 * 32 ** 3
    g = _gen(2000)
    src = torch.randn(N, C, generator=g)
    occupied = torch.randperm(cells, generator=g)[:9000]                 # ~5 points per occupied cell, most cells empty, as a gridded garment
    cell = occupied[torch.randint(0, 9000, (N,), generator=g)]
    src[N // 2:N // 2 + N // 8] = src[:N // 8]                          # equal rows in equal cells: ties
    cell[N // 2:N // 2 + N // 8] = cell[:N // 8]
    gout = torch.randn(cells, C, generator=g)
    clock = _CpuClock(f"grid_scatter[{reduce}]")
    fn = lambda s: s_scatter(s, cell, cells, reduce)                     # noqa: E731
    with clock:
        fwd64, (g64,) = _grads(fn, [src], gout, torch.float64)
    sd, cd = src.to(DEV), cell.to(torch.int32).to(DEV)
    vol = ops.grid_scatter(sd, cd, 1, (cells,), reduce)
    run = lambda: ops.grid_scatter_bwd(gout.to(DEV).view(vol.shape), cd, N, reduce, vol=vol, src=sd)     # noqa: E731
    gs = run()
    if reduce == "max":
        assert torch.equal(vol.view(cells, C).cpu(), fwd64.float())
        assert torch.equal(gs.cpu(), g64.float())
    else:
        with clock:
            _, (g32,) = _grads(fn, [src], gout, torch.float32)
        _check("full size grid_scatter[mean]", g64, g32, gs)
    assert torch.equal(gs, run())


def test_segment_max_bwd_at_24000_centres_65_slots_64_channels():
    """CPU side (fp64): 4.1 s (measured on the MI355X host; the whole test 4.7 s)"""
    M, S, C = 24000, 65, 64
    g = _gen(2010)
    h = torch.relu(torch.randn(M * S, C, generator=g))
    h[1::S] = h[0::S]                                                    # slot 1 repeats slot 0: ties
    slot = torch.randint(-20000, 48000, (M * S,), generator=g).to(torch.int32).clamp(min=-1)     # ~30 % empty slots
    slot[7 * S:8 * S] = -1
    gout = torch.randn(M, C, generator=g)
    with _CpuClock("segment_max"):
        fwd64, (g64,) = _grads(lambda t: s_segment_max(t, slot, M, S), [h], gout, torch.float64)
        fwd, want = fwd64.float(), g64.float()
        del fwd64, g64
    hd, sd = h.to(DEV), slot.to(DEV)
    out = ops.segment_max(hd, sd, M, S)
    assert torch.equal(out.cpu(), fwd)
    gh = ops.segment_max_bwd(gout.to(DEV), out, hd, sd, M, S)
    assert torch.equal(gh.cpu(), want)
    assert torch.equal(gh, ops.segment_max_bwd(gout.to(DEV), out, hd, sd, M, S))


def test_global_max_pool_bwd_at_8x3000_rows_256_channels():
    """CPU side (fp64): 0.2 s (measured on the MI355X host; the whole test 0.3 s)"""
    sizes, C = [3000] * 8, 256
    g = _gen(2020)
    h = torch.relu(torch.randn(sum(sizes), C, generator=g))
    h[2999] = h[15] = h[:3000].max(0).values + 1.0                       # above every other row; tied: row 15 wins over the last row of example 0
    gout = torch.randn(8, C, generator=g)
    with _CpuClock("global_max_pool"):
        fwd64, (g64,) = _grads(lambda t: s_global_max(t, sizes), [h], gout, torch.float64)
    seg = Segments(sizes, DEV)
    hd = h.to(DEV)
    out = ops.global_max_pool(hd, seg.ptr, seg.num)
    assert torch.equal(out.cpu(), fwd64.float())
    gh = ops.global_max_pool_bwd(gout.to(DEV), out, hd, seg.ptr, seg.num)
    assert torch.equal(gh.cpu(), g64.float()) and torch.equal(gh[15].cpu(), gout[0])
    assert torch.equal(gh, ops.global_max_pool_bwd(gout.to(DEV), out, hd, seg.ptr, seg.num))


def test_sa_gather_bwd_at_24000_centres_65_slots_64_channels():
    """CPU side (fp64 and fp32): 1.2 s (measured on the MI355X host; the whole test 1.7 s)"""
    n, Mc, S, C = 48000, 24000, 65, 64
    g = _gen(2030)
    slot = torch.randint(-20000, n, (Mc * S,), generator=g).to(torch.int32).clamp(min=-1)
    gout = torch.randn(Mc * S, C + 3, generator=g)
    pos, centre, x = torch.zeros(n, 3), torch.zeros(Mc, dtype=torch.int64), torch.zeros(n, C)
    fn = lambda t: s_sa_gather(t, pos.to(t.dtype), centre, slot, S)      # noqa: E731
    with _CpuClock("sa_gather"):
        _, (g64,) = _grads(fn, [x], gout, torch.float64)
        _, (g32,) = _grads(fn, [x], gout, torch.float32)
    gd, sd = gout.to(DEV), slot.to(DEV)
    gx = ops.sa_gather_bwd(gd, sd, C, n)
    _check("full size sa_gather", g64, g32, gx)
    assert torch.equal(gx, ops.sa_gather_bwd(gd, sd, C, n))


def test_knn_interpolate_bwd_at_24000_sources_48000_queries_128_channels():
    """CPU side (fp64 and fp32): 0.2 s (measured on the MI355X host; the whole test 0.3 s)"""
    src_sizes, q_sizes, C, k = [3000] * 8, [6000] * 8, 128, 3
    g = _gen(2040)
    pq = torch.rand(sum(q_sizes), 3, generator=g)
    ps = torch.cat([pq[6000 * b:6000 * b + 6000:2] for b in range(8)])  # the sources are every second query: d2 = 0 for half of the queries
    x, gout = torch.randn(sum(src_sizes), C, generator=g), torch.randn(sum(q_sizes), C, generator=g)
    sseg, qseg = Segments(src_sizes, DEV), Segments(q_sizes, DEV)
    nbr_d, d2_d = ops.knn_neighbours(ps.to(DEV), sseg.ptr, pq.to(DEV), qseg.ptr, k)
    nbr, d2 = nbr_d.cpu(), d2_d.cpu()
    fn = lambda t: s_knn(t, nbr, d2)                                     # noqa: E731
    with _CpuClock("knn_interpolate"):
        fwd64, (g64,) = _grads(fn, [x], gout, torch.float64)
        _, (g32,) = _grads(fn, [x], gout, torch.float32)
    out = ops.knn_interpolate(x.to(DEV), ps.to(DEV), sseg.ptr, pq.to(DEV), qseg.ptr, k)
    assert torch.allclose(out.cpu().double(), fwd64, rtol=1e-5, atol=1e-5)
    gd = gout.to(DEV)
    gx = ops.knn_interpolate_bwd(gd, nbr_d, d2_d, sum(src_sizes))
    _check("full size knn_interpolate", g64, g32, gx)
    assert torch.equal(gx, ops.knn_interpolate_bwd(gd, nbr_d, d2_d, sum(src_sizes)))


def test_trilinear_sample_bwd_at_24x6000_queries_into_32cubed_x128():
    """CPU side (fp64 and fp32): 0.4 s (measured on the MI355X host; the whole test, which also draws the 100 M-element volume, 2.1 s)"""
    B, M, C, G = 24, 6000, 128, 32
    g = _gen(2050)
    vol = torch.randn(B, G, G, G, C, generator=g)                        # channel-last, as the kernel reads it
    q = torch.rand(B, M, 3, generator=g) * 1.1 - 0.05                   # a few beyond the borders
    q[:, :1500] = 0.5 + 0.02 * torch.randn(B, 1500, 3, generator=g)     # a dense clump: a few voxels read by hundreds of queries
    # keep every query 1e-3 of a voxel away from the lattice planes: grad_query is the slope INSIDE a cell and jumps across a plane, and with
    # 432 000 coordinates one of them would otherwise sit within an fp32 rounding error (2e-6 at index 16..31) of a plane, where the fp32 and the
    # fp64 run of the restatement differentiate different cells and the measured e32 says nothing about rounding
    x = q.double() * (G - 1)
    q[(x - x.round()).abs() < 1e-3] += 2e-3 / (G - 1)
    x = q.double() * (G - 1)
    assert float((x - x.round()).abs().min()) > 5e-4
    gout = torch.randn(B, M, C, generator=g)
    volc = vol.permute(0, 4, 1, 2, 3)
    with _CpuClock("trilinear_sample"):
        _, (gv64, gq64) = _grads(r_sample, [volc, q], gout, torch.float64)
        _, (gv32, gq32) = _grads(r_sample, [volc, q], gout, torch.float32)
    vd, qd, gd = vol.to(DEV), q.to(DEV), gout.to(DEV)
    gv, gq = ops.trilinear_sample_bwd(gd, vd, qd, want_vol=True, want_query=True)
    _check("full size trilinear_sample grad_vol", gv64.permute(0, 2, 3, 4, 1), gv32.permute(0, 2, 3, 4, 1), gv)
    _check("full size trilinear_sample grad_query", gq64, gq32, gq)
    gv2, gq2 = ops.trilinear_sample_bwd(gd, vd, qd, want_vol=True, want_query=True)
    assert torch.equal(gv, gv2) and torch.equal(gq, gq2)
