"""GPU (-m gpu): train-mode BatchNorm for the MLP blocks -- gn_col_moments, gn_col_dots, gn_bn_train_bwd (csrc/linear_grad.hip) and
autograd.mlp / implicit_decode with batch_stats=True.

Directly called kernels, each on contiguous operands and on column slices of wider NaN-filled buffers (the two must agree bit for bit, no NaN may leak,
the pads stay NaN), every output computed twice for bit equality.  u = 2^-53 throughout.
    gn_col_moments (two passes: mean = sum / M, then the squares of the fp64 differences from it), against numpy's fp64 two-pass:
        every summation order of M fp64 terms errs by at most M u sum |term|, so the computed mean is off by d <= M u mean|r| + u |mean| (the sum, the
        division) and m2 by at most (M + 4) u m2 + M d^2: (M - 1) additions, three roundings per term (the difference, the square, its conversion are one
        each at most), and sum (r - mean - e)^2 = m2 + M e^2 for a mean off by e.  numpy's own two-pass has the same worst case, so the test allows
        twice each.  What the bound implies for inv = 1 / sqrt(m2 / M + eps): a relative error of at most (M + 4) u / 2 + d^2 / (2 var); where the
        variance is at least 1e-6 of the mean square, d^2 / var <= ((M + 1) u)^2 * 1e6, so at M = 1.6 M rows inv is good to 2^-32, at this file's
        M <= 8193 to 2^-40 (asserted below: below 2^-30).  Constant columns (one all zero) give mean == c and m2 == 0.0 exactly; a column 1e4 + unit
        noise stays inside the bound.
    gn_col_dots and gn_bn_train_bwd's sum_g: the terms are exact fp64 numbers, only the order differs from the exactly rounded sum (math.fsum):
        |ours - sum| <= M u sum |term|.
    gn_bn_train_bwd's g: numpy's fp64 (a * dy + b * r) + c rounded once to fp32, 1 fp32 ulp allowed; exact +0 under the mask (r <= 0, -0, NaN).

Stacks with batch_stats=True: the error rule of tests/grad_reference.py::_check (ours against torch-fp64 on the CPU at most 4 x (torch-fp32 on the CPU
against fp64) + 1 fp32 ulp of the largest entry) for the forward y and every gradient; the reference is F.linear -> the HIP forward's own ReLU mask ->
F.batch_norm(training=True).  The running buffers are held to nn.BatchNorm1d in fp64, fed the HIP forward's own r, rounded to fp32, within 2 ulp.

Mutation record (one-line mutants of the new code and the test written to catch each; reasoning only -- none of the mutant builds has been run on a GPU):
    1. unbiased instead of biased variance in inv (m2 / (M - 1) in _batch_stats_forward): test_stack[*] (y and every gradient; at 700-1100 rows the
       change is 1e-3 relative, four orders above the bound).
    2. a dropped `- b * mean` in c (_bn_bwd_coef): tests/test_bn_train_host.py's closed forms without a GPU; here test_stack[*] (d x, d weight).
    3. the mask taken from y instead of r (y > 0 in gn_bn_train_bwd's call): test_bn_train_bwd_direct cannot see it (the kernel has no y); test_stack[*]
       through the negative gamma of the first block (y > 0 exactly where r is 0) and the dead column (y = beta > 0 for half the seeds).
    4. M - 1 swapped in the running update (m2 / M into running_var): test_stack[*] buffers (0.1 * var / M is 1e3 ulp); the host test without a GPU.
    5. a reversed run order in the fold (run 7 first): bit equality alone cannot see it; the bounds do not either (any order meets them) -- the order is
       documentation, held only by the kernel's text.  Not caught.
    6. the halving tree starting at h = groups instead of groups / 2 (reads past the group table): out of the red[] array -- not run.
    7. CS_M2 reading p[0] instead of p[n] (every column centred on column 0's mean): test_col_moments_direct at N > 1 (m2 of the offset column, the
       constant column no longer 0.0).
    8. cw fixed at 64 with grp = tid / 64 but groups = 256 / cw left (rows skipped at N < 64): test_col_*_direct at N in {1, 3}.
    9. the second chunk's partial written over the first (part index without blockIdx.x): every direct test at M > chunk.
"""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from garmentnets_amd import _lib, autograd as A, ops  # noqa: E402
from garmentnets_amd.components.mlp import MLP, fold_batchnorm  # noqa: E402
from garmentnets_amd.components.pointnet2 import Segments  # noqa: E402
from garmentnets_amd.networks.conv_implicit_wnf import ImplicitWNFDecoder  # noqa: E402
from grad_reference import _check, _gen, _randomise_norms, r_sa_gather, r_sample, r_segment_max  # noqa: E402

DEV = "cuda:0"
RA = _lib.LINEAR_ACT_CHUNK_ROWS
NAN = float("nan")
U = 2.0 ** -53
MS = [2, RA - 1, RA, RA + 1, 8 * RA + 1]
NS = [1, 3, 63, 64, 65, 129]


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _embed(t, ld, off=0):
    """t as a column slice [off, off + cols) of a NaN-filled buffer of ld columns, on the GPU: (the slice, the buffer)"""
    buf = torch.full((t.shape[0], ld), NAN, dtype=t.dtype)
    buf[:, off:off + t.shape[1]] = t
    buf = buf.to(DEV)
    return buf[:, off:off + t.shape[1]], buf


def _pads_are_nan(buf, off, n):
    return bool(torch.isnan(buf[:, :off]).all()) and bool(torch.isnan(buf[:, off + n:]).all())


def _exact_colsum(t):
    """the exactly rounded column sums of an fp64 array [M][N]"""
    return np.array([math.fsum(col) for col in np.ascontiguousarray(t.T)])


# ------------------------------------------------------------------------------------------------ 1. the kernels, directly
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_col_moments_direct(M, N):
    """the bound of the module docstring; r = relu(.) (many zeros); the last column 1e4 + unit noise, the one before it constant 0.37, the one before
    that all zero (as far as N has them); then whole matrices of one value"""
    g_ = _gen(1000 * M + N)
    r = torch.relu(torch.randn(M, N, generator=g_) + 0.3)
    if N >= 2:
        r[:, N - 1] = 1e4 + torch.randn(M, generator=g_)
    if N >= 3:
        r[:, N - 2] = 0.37
        r[:, N - 3] = 0.0
    out = ops.col_moments(r.to(DEV))
    assert out.dtype == torch.float64 and tuple(out.shape) == (2, N)
    rd, rbuf = _embed(r, N + 7, 2)
    assert _same_bits(ops.col_moments(rd), out) and _pads_are_nan(rbuf, 2, N)
    assert _same_bits(ops.col_moments(r.to(DEV)), out)
    mean, m2 = out.cpu().numpy()
    r64 = r.double().numpy()
    mean_ref = r64.sum(0) / M
    m2_ref = ((r64 - mean_ref) ** 2).sum(0)
    d = M * U * np.abs(r64).mean(0) + U * np.abs(mean_ref)
    m2_bound = (M + 4) * U * m2_ref + M * d * d
    e_mean, e_m2 = np.abs(mean - mean_ref), np.abs(m2 - m2_ref)
    print(f"[bn-train] col_moments M={M} N={N}: mean error / bound {float((e_mean / np.maximum(2 * d, 1e-300)).max()):.3e}, "
          f"m2 error / bound {float((e_m2 / np.maximum(2 * m2_bound, 1e-300)).max()):.3e}")
    assert np.isfinite(mean).all() and np.isfinite(m2).all()
    assert (e_mean <= 2 * d).all() and (e_m2 <= 2 * m2_bound).all()
    # what the (one-sided) bound implies for inv where the variance is at least 1e-6 of the mean square
    assert (M + 4) * U / 2 + ((M + 1) * U) ** 2 * 1e6 / 2 < 2.0 ** -30
    if N >= 3:
        assert mean[N - 2] == np.float32(0.37) and m2[N - 2] == 0.0 and mean[N - 3] == 0.0 and m2[N - 3] == 0.0
        assert e_m2[N - 1] <= 2 * m2_bound[N - 1] and m2_ref[N - 1] > 0                     # the offset column: inside the bound
    for c in (0.0, 0.37, -1e4):
        mc = ops.col_moments(torch.full((M, N), c).to(DEV)).cpu().numpy()
        assert (mc[0] == np.float32(c)).all() and (mc[1] == 0.0).all(), c


def _sum_check(tag, ours, terms, M):
    want = _exact_colsum(terms)
    bound = M * U * _exact_colsum(np.abs(terms))
    err = np.abs(ours - want)
    print(f"[bn-train] {tag}: largest error {float(err.max()):.3e}, largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3e}")
    assert np.isfinite(ours).all() and (err <= bound).all(), tag


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_col_dots_direct(M, N):
    g_ = _gen(2000 * M + N)
    dy = torch.randn(M, N, generator=g_)
    r = torch.relu(torch.randn(M, N, generator=g_) + 0.3)
    out = ops.col_dots(dy.to(DEV), r.to(DEV))
    assert out.dtype == torch.float64 and tuple(out.shape) == (2, N)
    dyd, dybuf = _embed(dy, N + 3)
    rd, rbuf = _embed(r, N + 7, 2)
    assert _same_bits(ops.col_dots(dyd, rd), out) and _pads_are_nan(dybuf, 0, N) and _pads_are_nan(rbuf, 2, N)
    assert _same_bits(ops.col_dots(dy.to(DEV), r.to(DEV)), out)
    ours = out.cpu().numpy()
    _sum_check(f"col_dots M={M} N={N} sum dy", ours[0], dy.double().numpy(), M)
    _sum_check(f"col_dots M={M} N={N} sum dy * r", ours[1], dy.double().numpy() * r.double().numpy(), M)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_bn_train_bwd_direct(M, N):
    """coef with a zero and a negative a; r = relu(.) with -0, a denormal and one NaN planted"""
    g_ = _gen(3000 * M + N)
    dy = torch.randn(M, N, generator=g_)
    r = torch.relu(torch.randn(M, N, generator=g_) + 0.3)
    special = torch.tensor([NAN, -0.0, 1e-42])[:M * N]
    r.view(-1)[:special.numel()] = special
    coef = torch.randn(3, N, generator=g_, dtype=torch.float64)
    coef[0, 0] = -1.3
    if N > 1:
        coef[0, N - 1] = 0.0
    cd = coef.to(DEV)
    g, sum_g = ops.bn_train_bwd(dy.to(DEV), r.to(DEV), cd)
    assert g.dtype == torch.float32 and tuple(g.shape) == (M, N) and sum_g.dtype == torch.float64 and tuple(sum_g.shape) == (N,)
    # the fp64 formula, each operation rounded (no contraction), then once to fp32
    a, b, c = coef.numpy()
    with np.errstate(invalid="ignore"):
        full = ((a * dy.double().numpy() + b * r.double().numpy()) + c).astype(np.float32)
    on = r.numpy() > 0
    gh = g.cpu().numpy()
    assert not np.isnan(gh).any()
    assert not gh.view(np.int32)[~on].any()                                       # exact +0 under the mask: r <= 0, -0 and the NaN
    assert gh.reshape(-1)[0] == 0.0 and (M * N < 3 or gh.reshape(-1)[2] != 0.0 or full.reshape(-1)[2] == 0.0)      # the NaN takes none, the denormal does
    err = np.abs(gh.astype(np.float64) - full.astype(np.float64))[on]
    assert (err <= np.spacing(np.abs(full[on])).astype(np.float64)).all()
    print(f"[bn-train] bn_train_bwd M={M} N={N}: {int((err > 0).sum())} of {int(on.sum())} unmasked entries differ from numpy's (by at most 1 ulp)")
    _sum_check(f"bn_train_bwd M={M} N={N} sum g", sum_g.cpu().numpy(), gh.astype(np.float64), M)
    # column slices of wider NaN-filled buffers, each at its own offset and stride
    dyd, dybuf = _embed(dy, N + 3)
    rd, rbuf = _embed(r, N + 7, 2)
    gout, gbuf = _embed(torch.zeros(M, N), N + 5, 4)
    g2, sum2 = ops.bn_train_bwd(dyd, rd, cd, out=gout)
    assert g2.data_ptr() == gout.data_ptr() and _same_bits(g2, g) and _same_bits(sum2, sum_g)
    assert _pads_are_nan(gbuf, 4, N) and _pads_are_nan(dybuf, 0, N) and _pads_are_nan(rbuf, 2, N)
    # g aliasing dy
    g3, sum3 = ops.bn_train_bwd(dyd, rd, cd, out=dyd)
    assert g3.data_ptr() == dyd.data_ptr() and _same_bits(g3, g) and _same_bits(sum3, sum_g) and _pads_are_nan(dybuf, 0, N)
    # twice
    g4, sum4 = ops.bn_train_bwd(dy.to(DEV), r.to(DEV), cd)
    assert _same_bits(g4, g) and _same_bits(sum4, sum_g)


def test_no_rows_write_zeros():
    e = torch.empty(0, 5, device=DEV)
    assert not bool(_bits(ops.col_moments(e)).any()) and not bool(_bits(ops.col_dots(e, e)).any())
    g, s = ops.bn_train_bwd(e, e, torch.ones(3, 5, dtype=torch.float64, device=DEV))
    assert tuple(g.shape) == (0, 5) and not bool(_bits(s).any())


# ------------------------------------------------------------------------------------------------ 2. stacks
def _stack(channels, seed):
    """a training-mode MLP: random BatchNorm parameters and buffers, in the first block a negative and a zero gamma (_randomise_norms) and a dead column
    (a large negative Linear bias: r == 0 in every row of column 2)"""
    torch.manual_seed(seed)
    stack = MLP(channels)
    _randomise_norms(stack, _gen(seed + 1000))
    with torch.no_grad():
        stack[0][0].bias[2] = -1e3
    return stack.train()


def hip_forward(stack_gpu, rows):
    """the blocks of A.mlp(stack, rows, batch_stats=True) one by one ON A COPY of the stack (its buffers are updated, the caller's are not): the saved
    r of every block (CPU) and the result"""
    sg = copy.deepcopy(stack_gpu)
    rs, h = [], rows
    with torch.no_grad():
        for block in sg:
            lin, bn = block[0], block[2]
            wp = torch.zeros(lin.out_features, ops.pad4(lin.in_features), device=DEV)
            wp[:, :lin.in_features] = lin.weight
            if bn.training:
                r, h = A._batch_stats_forward(h, wp, lin.bias.detach(), lin.in_features, bn)[:2]
            else:
                r = ops.linear(h, wp, lin.bias.detach(), None, None, relu=True, K=lin.in_features)
                h = ops.row_affine(r, *fold_batchnorm(bn))
            rs.append(r.cpu())
    return rs, h


def r_mlp(stack, P, h, masks, prefix=""):
    """the restatement: F.linear -> the handed-in ReLU mask -> F.batch_norm, training (batch statistics) or eval (the module's running statistics, as they
    are when this is called) by each module's own mode.  stack: the CPU module; P: its parameters in h's dtype"""
    for i, block in enumerate(stack):
        bn = block[2]
        r = F.linear(h, P[f"{prefix}{i}.0.weight"], P[f"{prefix}{i}.0.bias"]) * masks[i].to(h.dtype)
        rm, rv = (None, None) if bn.training else (bn.running_mean.to(h.dtype), bn.running_var.to(h.dtype))
        h = F.batch_norm(r, rm, rv, P[f"{prefix}{i}.2.weight"], P[f"{prefix}{i}.2.bias"], bn.training, 0.0, bn.eps)
    return h


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def _params(module, dtype, prefix=""):
    return {prefix + k: p.detach().to(dtype).requires_grad_(True) for k, p in module.named_parameters()}


def restated(stack, x, dy, dtype, masks):
    P = _params(stack, dtype)
    xx = _leaf(x, dtype)
    y = r_mlp(stack, P, xx, masks)
    return y.detach(), dict(zip(["x"] + list(P), torch.autograd.grad(y, [xx] + list(P.values()), dy.to(dtype))))


def hip_run(stack_gpu, x, dy, before_backward=None):
    xg = x.to(DEV).requires_grad_(True)
    y = A.mlp(stack_gpu, xg, batch_stats=True)
    if before_backward is not None:
        before_backward()
    names = ["x"] + [k for k, _ in stack_gpu.named_parameters()]
    return y.detach(), dict(zip(names, torch.autograd.grad(y, [xg] + list(stack_gpu.parameters()), dy.to(DEV))))


def _compare(tag, y64, y32, yh, g64, g32, gh):
    assert set(gh) == set(g64), (tag, sorted(gh), sorted(g64))
    return max([_check(f"{tag} y", y64, y32, yh)] + [_check(f"{tag} d {k}", g64[k], g32[k], gh[k]) for k in g64])


def _buffers(stack):
    return {k: b.detach().clone() for k, b in stack.named_buffers()}


def _check_buffers(tag, stack_gpu, before, rs):
    """one call: every BatchNorm of the stack against nn.BatchNorm1d in fp64, started from the fp32 buffers `before` and fed the HIP forward's own r
    (rs: one per block), rounded to fp32: 2 ulp; an eval-mode module keeps its bits"""
    for i, block in enumerate(stack_gpu):
        bn = block[2]
        if not bn.training:
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                assert torch.equal(getattr(bn, k).cpu(), before[f"{i}.2.{k}"].cpu()), (tag, i, k)
            continue
        ref = torch.nn.BatchNorm1d(bn.num_features, eps=bn.eps, momentum=bn.momentum).double()
        with torch.no_grad():
            ref.running_mean.copy_(before[f"{i}.2.running_mean"])
            ref.running_var.copy_(before[f"{i}.2.running_var"])
            ref.num_batches_tracked.copy_(before[f"{i}.2.num_batches_tracked"])
            ref(rs[i].double())
        assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == int(before[f"{i}.2.num_batches_tracked"]) + 1, (tag, i)
        for k in ("running_mean", "running_var"):
            got, want = getattr(bn, k).cpu().numpy(), getattr(ref, k).float().numpy()
            print(f"[bn-train] {tag} block {i} {k}: largest difference {float((np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want))).max()):.1f} ulp")
            assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - want) <= 2 * np.spacing(np.abs(want))).all(), (tag, i, k)


STACKS = {"sa1": ([6, 64, 64, 128], 1000), "sa2": ([131, 128, 128, 256], 700), "dec1": ([128, 256, 256, 1], 1100)}


@pytest.mark.parametrize("which", list(STACKS))
def test_stack(which):
    channels, rows = STACKS[which]
    seed = sum(map(ord, which))
    stack = _stack(channels, seed)
    sg = copy.deepcopy(stack).to(DEV)
    g_ = _gen(seed + 1)
    x, x2 = torch.randn(rows, channels[0], generator=g_), torch.randn(rows, channels[0], generator=g_)
    dy = torch.randn(rows, channels[-1], generator=g_)
    before = _buffers(sg)
    rs, fwd = hip_forward(sg, x.to(DEV))
    assert not bool(rs[0][:, 2].any())                                          # the dead column
    masks = [r > 0 for r in rs]
    y, gh = hip_run(sg, x, dy)
    assert _same_bits(y, fwd), which
    (y64, g64), (y32, g32) = (restated(stack, x, dy, dt, masks) for dt in (torch.float64, torch.float32))
    _compare(f"bn-train stack {which}", y64, y32, y, g64, g32, gh)
    _check_buffers(which, sg, before, rs)
    after_one = _buffers(sg)
    # a run whose buffers are put back before the backward: the same bits (the backward reads the captured statistics, not the buffers)
    fresh = copy.deepcopy(stack).to(DEV)

    def restore():
        with torch.no_grad():
            for k, b in fresh.named_buffers():
                b.copy_(before[k])
    y_r, gh_r = hip_run(fresh, x, dy, before_backward=restore)
    assert _same_bits(y_r, y) and all(_same_bits(gh_r[k], gh[k]) for k in gh), which
    # under no_grad: the same y, the same buffers, nothing saved
    quiet = copy.deepcopy(stack).to(DEV)
    with torch.no_grad():
        y_q = A.mlp(quiet, x.to(DEV).requires_grad_(True), batch_stats=True)
    assert not y_q.requires_grad and y_q.grad_fn is None and _same_bits(y_q, y), which
    assert all(_same_bits(b, after_one[k]) if b.is_floating_point() else torch.equal(b, after_one[k]) for k, b in quiet.named_buffers()), which
    # when nothing requires a gradient, the same again
    frozen = copy.deepcopy(stack).to(DEV).requires_grad_(False)
    y_f = A.mlp(frozen, x.to(DEV), batch_stats=True)
    assert not y_f.requires_grad and _same_bits(y_f, y), which
    assert all(_same_bits(b, after_one[k]) if b.is_floating_point() else torch.equal(b, after_one[k]) for k, b in frozen.named_buffers()), which
    # a second call starts from the updated buffers; leading dimensions (B, M, C) are flattened
    rs2, fwd2 = hip_forward(sg, x2.to(DEV))
    y2, gh2 = hip_run(sg, x2.view(2, rows // 2, -1), dy.view(2, rows // 2, -1))
    assert tuple(y2.shape) == (2, rows // 2, channels[-1]) and _same_bits(y2.reshape(rows, -1), fwd2), which
    _check_buffers(which + " second call", sg, after_one, rs2)                  # (from the fp32 buffers the first call left, as a module holds them)
    assert all(int(block[2].num_batches_tracked) == 2 for block in sg), which
    assert tuple(gh2["x"].shape) == (2, rows // 2, channels[0]), which


def test_mixed_stack_each_block_follows_its_own_mode():
    """block 0 in eval mode (its running statistics, its buffers untouched), block 1 training"""
    channels, rows = [20, 48, 33], 600
    stack = _stack(channels, 77)
    stack[0][2].eval()
    sg = copy.deepcopy(stack).to(DEV)
    assert not sg[0][2].training and sg[1][2].training
    g_ = _gen(78)
    x, dy = torch.randn(rows, channels[0], generator=g_), torch.randn(rows, channels[-1], generator=g_)
    before = _buffers(sg)
    rs, fwd = hip_forward(sg, x.to(DEV))
    masks = [r > 0 for r in rs]
    y, gh = hip_run(sg, x, dy)
    assert _same_bits(y, fwd)
    (y64, g64), (y32, g32) = (restated(stack, x, dy, dt, masks) for dt in (torch.float64, torch.float32))
    _compare("bn-train mixed stack", y64, y32, y, g64, g32, gh)
    _check_buffers("mixed", sg, before, rs)
    y2, gh2 = hip_run(copy.deepcopy(stack).to(DEV), x, dy)
    assert _same_bits(y2, y) and all(_same_bits(gh2[k], gh[k]) for k in gh)


# ------------------------------------------------------------------------------------------------ 3. compositions
def test_point_conv_max_with_batch_statistics_over_all_edge_rows():
    """PointConv(local_nn = autograd.mlp(stack, batch_stats=True), aggr='max') on 300 points, K = 16: the statistics run over all Mc * (K + 1) edge rows,
    self loops and the zero rows of empty slots included.  The ReLU masks are the HIP forward's, the max winners each side's own."""
    n, C, K = 300, 13, 16
    g_ = _gen(131)
    pos, x = torch.rand(n, 3, generator=g_), torch.randn(n, C, generator=g_)
    stack = _stack([C + 3, 32, 24], 132)
    sg = copy.deepcopy(stack).to(DEV)
    pd = pos.to(DEV)
    seg0 = Segments([n], DEV)
    idx = A.fps(pd, seg0, 0.5)
    seg1 = Segments([ops.fps_count(n, 0.5)], DEV)
    nbr, _ = A.ball_table(pd, idx, 0.25, seg0, seg1, K)
    Mc, S = nbr.shape[0], K + 1
    with torch.no_grad():
        edges, slot, _ = ops.sa_gather(x.to(DEV), pd, idx.to(torch.int32), nbr)
    assert edges.shape[0] == Mc * S
    rs, _ = hip_forward(sg, edges)
    masks = [r > 0 for r in rs]
    slot = slot.cpu()
    dy = torch.randn(Mc, 24, generator=g_)
    before = _buffers(sg)

    def hip(module):
        xg = x.to(DEV).requires_grad_(True)
        out = A.point_conv_max(xg, pd, idx, nbr, lambda e: A.mlp(module, e, batch_stats=True))
        return out.detach(), dict(zip(["x"] + [k for k, _ in module.named_parameters()], torch.autograd.grad(out, [xg] + list(module.parameters()), dy.to(DEV))))
    res = {}
    for dt in (torch.float64, torch.float32):
        P = _params(stack, dt)
        xx = _leaf(x, dt)
        out = r_segment_max(r_mlp(stack, P, r_sa_gather(xx, pos.to(dt), idx.cpu(), slot, S), masks), slot, Mc, S)
        res[dt] = (out.detach(), dict(zip(["x"] + list(P), torch.autograd.grad(out, [xx] + list(P.values()), dy.to(dt)))))
    yh, gh = hip(sg)
    _compare("bn-train point_conv_max(mlp)", res[torch.float64][0], res[torch.float32][0], yh, res[torch.float64][1], res[torch.float32][1], gh)
    _check_buffers("point_conv_max", sg, before, rs)
    yh2, gh2 = hip(copy.deepcopy(stack).to(DEV))
    assert _same_bits(yh2, yh) and all(_same_bits(gh2[k], gh[k]) for k in gh)


def test_implicit_decode_with_batch_statistics():
    """autograd.implicit_decode(..., batch_stats=True) on an 8^3 x 16 volume with 500 queries (drawn in [-0.1, 1.1]: some clamp at the border): gradients
    to the volume, the queries and every parameter"""
    g_ = _gen(141)
    B, C, G, Mq = 1, 16, 8, 500
    torch.manual_seed(142)
    dec = ImplicitWNFDecoder(nn_channels=(C, 64, 64, 1))
    _randomise_norms(dec, _gen(143))
    with torch.no_grad():
        dec.mlp[0][0].bias[2] = -1e3
    dec.train()
    dg = copy.deepcopy(dec).to(DEV)
    vol = torch.randn(B, C, G, G, G, generator=g_)
    q = torch.rand(B, Mq, 3, generator=g_) * 1.2 - 0.1
    dy = torch.randn(B, Mq, 1, generator=g_)
    with torch.no_grad():
        rows = A.grid_sample_points(vol.to(DEV), q.to(DEV))
    rs, _ = hip_forward(dg.mlp, rows.reshape(-1, C))
    masks = [r > 0 for r in rs]
    before = _buffers(dg.mlp)

    def hip(module):
        vg, qg = vol.to(DEV).requires_grad_(True), q.to(DEV).requires_grad_(True)
        y = A.implicit_decode(module, vg, qg, batch_stats=True)
        assert tuple(y.shape) == (B, Mq, 1)
        names = ["volume", "query"] + ["mlp." + k for k, _ in module.mlp.named_parameters()]
        return y.detach(), dict(zip(names, torch.autograd.grad(y, [vg, qg] + list(module.mlp.parameters()), dy.to(DEV))))
    res = {}
    for dt in (torch.float64, torch.float32):
        P = _params(dec.mlp, dt, "mlp.")
        vv, qq = _leaf(vol, dt), _leaf(q, dt)
        y = r_mlp(dec.mlp, P, r_sample(vv, qq).reshape(-1, C), masks, "mlp.").reshape(B, Mq, 1)
        res[dt] = (y.detach(), dict(zip(["volume", "query"] + list(P), torch.autograd.grad(y, [vv, qq] + list(P.values()), dy.to(dt)))))
    yh, gh = hip(dg)
    _compare("bn-train implicit_decode", res[torch.float64][0], res[torch.float32][0], yh, res[torch.float64][1], res[torch.float32][1], gh)
    _check_buffers("implicit_decode", dg.mlp, before, rs)
    yh2, gh2 = hip(copy.deepcopy(dec).to(DEV))
    assert _same_bits(yh2, yh) and all(_same_bits(gh2[k], gh[k]) for k in gh)
    # without the keyword a training decoder is still refused
    with pytest.raises(NotImplementedError, match="train-mode BatchNorm"):
        A.implicit_decode(dg, vol.to(DEV), q.to(DEV))
