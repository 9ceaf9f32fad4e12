"""GPU (-m gpu): gradients of the MLP blocks (csrc/linear_grad.hip, autograd.mlp / linear / implicit_decode).

Reference: a plain-torch restatement of one block -- F.linear -> relu -> eval-mode F.batch_norm, on the module's own parameters -- run on the CPU in
fp64 and in fp32 (tests/test_mlp_grad_host.py pins its gradients to the closed forms the kernels implement).  Error rule
(tests/grad_reference.py::_check): ours against fp64 at most 4 x (torch-fp32 against fp64) + 1 fp32 ulp of the largest gradient, printed as
`[grad-error] ...` before it is asserted.  No element is excluded.

Block, stack, A.linear, decoder and production-shape tests hand the restatement the ReLU masks of the HIP forward (the saved r > 0, read by running the
same kernels: hip_masks), so both sides differentiate the same piecewise-linear map and a ReLU that flips between fp32 and fp64 does not blur the
measure.  The two compositions that contain other selections (PointConv's max, the UNet) let each side form its own, as the suites of those operators do.

Directly called kernels are held to bounds derived from their own summation:
    gn_linear_act_bwd: g bit-equal to torch.where(r > 0, dy * sc, 0) in fp32; the sums add exact fp64 products, so only the fp64 summation order
        differs from the reference: |ours - ref| <= M * 2^-52 * sum |term| per entry.
    gn_linear_bwd_weight: at most R sequential fp32 fmas per chunk (R = _lib.LINEAR_BWD_CHUNK_ROWS), the chunks folded in fp64, one rounding:
        |ours - fp64| <= (R + 2) * 2^-24 * (|g|^T |x|) elementwise.  Beside it the rule at factor 4 against torch-fp32 (the final convolution's shapes came here with it).

Production shapes (test_production_shape): only the fp64 side costs time; measured on the test machine, the whole test (both restatements, two HIP
runs) took 1.2 s at 144 000 x 128 -> 256 and 0.3 s at 48 000 x 137 -> 137.  The largest ours / torch-fp32 figure of each family is kept in DESIGN.md
"MLP gradients".

Mutation record.  Five one-line mutants of csrc/linear_grad.hip, each staying inside every buffer this file hands the kernels, and the tests that are
written to catch them.  The mutant builds have NOT been run on a GPU yet: the column "caught by" is the reasoning, to be replaced by the observed list.
    1. the half-wave row offset (aoff = 0 * BN + ...: both half-waves feed row m of g, so g[m + 1] is dropped and g[m] * x[m + 1] enters): every
       test_linear_bwd_weight_direct case with M > 1 (the derived bound), test_stack_gradients, test_production_shape.
    2. a tail guard (stages = floor((m1 - m0) / 16): the ragged last stage of a chunk is dropped): test_linear_bwd_weight_direct[7-3-5, 65-33-31,
       R+1-128-131, 2R+7-*, 3R-1-257-64, 130-1024-1280] (and, added with the final convolution's shapes, [1031-8-32-ldx40, 2061-128-32, 300-512-7, 520-5-1023]) -- [4R-128-32] holds whole stages and must pass; [1-1-1] keeps its one stage (the mutant
       clamps at one) and must pass.
    3. the chunk stride of the partials (the fold reads part[c * (total - 1) + o]): test_linear_bwd_weight_direct cases with more than one chunk
       ([R+1-128-131], [2R+7-*], [3R-1-257-64], [4R-128-32]) and test_linear_act_bwd_direct[2051-257] (three chunks); harmless by construction with one
       chunk (c = 0).
    4. the mask comparison (r >= 0 in place of r > 0): test_linear_act_bwd_direct at every shape (the +0 / -0 of r: g must be 0 there), bit for bit.
    5. a swapped stride (r read with dy's row stride): test_linear_act_bwd_direct with M > 1 and r given (lddy = N + 3, ldr = N + 7); the stack tests
       where the width is no multiple of 4 (dy rows of N floats, r rows of pad4(N)): [agg] (137), [dec1], [dec3]; harmless by construction where
       both strides are equal (widths that are multiples of 4 with contiguous gradients).
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from garmentnets_amd import _lib, arith as AR, autograd as A, ops  # noqa: E402
from garmentnets_amd.components.mlp import MLP, HipLinear, param_cache  # noqa: E402
from garmentnets_amd.components.pointnet2 import Segments  # noqa: E402
from garmentnets_amd.components.unet3d import Abstract3DUNet  # noqa: E402
from garmentnets_amd.networks.conv_implicit_wnf import ImplicitWNFDecoder  # noqa: E402
from grad_reference import _check, _gen, _randomise_norms, r_sa_gather, r_sample, r_segment_max, r_unet  # noqa: E402

DEV = "cuda:0"
R = _lib.LINEAR_BWD_CHUNK_ROWS
RA = _lib.LINEAR_ACT_CHUNK_ROWS
NAN = float("nan")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _embed(t, ld, off=0):
    """t as a column slice [off, off + cols) of a NaN-filled buffer of ld columns, on the GPU: (the slice, the buffer)"""
    buf = torch.full((t.shape[0], ld), NAN, dtype=t.dtype)
    buf[:, off:off + t.shape[1]] = t
    buf = buf.to(DEV)
    return buf[:, off:off + t.shape[1]], buf


# ------------------------------------------------------------------------------------------------ 1. gn_linear_act_bwd, directly
# (1031, 8) and (300, 512): the bias gradient of the UNet's final convolution (the call without r and sc) at the widths of WEIGHT_CASES' final-conv shapes
@pytest.mark.parametrize("M,N", [(1, 1), (5, 3), (257, 65), (1031, 128), (2 * RA + 3, 257), (1031, 8), (300, 512)])
def test_linear_act_bwd_direct(M, N):
    """padded strides (dy, r and g each a slice of a wider NaN-filled buffer); sc with a negative entry and an exact 0; r = relu(.) (many +0) with -0, a
    denormal and one NaN planted.  (1, 1) holds one value: its sc is the negative one, its r the +0."""
    g_ = _gen(100 * M + N)
    dy = torch.randn(M, N, generator=g_)
    r = torch.relu(torch.randn(M, N, generator=g_))
    special = torch.tensor([0.0, -0.0, 1e-42, NAN])[:M * N]
    r.view(-1)[:special.numel()] = special
    if M * N > 8:
        r.view(-1)[-3:] = special[1:]
    sc = torch.randn(N, generator=g_)
    sc[0] = -1.5
    if N > 1:
        sc[N - 1] = 0.0
    dyd, dybuf = _embed(dy, N + 3)
    rd, _ = _embed(r, N + 7, 2)
    scd = sc.to(DEV)
    zero = torch.zeros(())
    for with_r, with_sc in ((True, True), (False, True), (True, False), (False, False)):
        tag = f"act_bwd M={M} N={N} r={with_r} sc={with_sc}"
        gout, gbuf = _embed(torch.zeros(M, N), N + 5, 4)
        run = lambda: ops.linear_act_bwd(dyd, rd if with_r else None, scd if with_sc else None, out=gout if (with_r or with_sc) else None)  # noqa: E731
        g, sums = run()
        assert sums.dtype == torch.float64 and tuple(sums.shape) == (3, N)
        ref = dy * sc if with_sc else dy
        if with_r:
            ref = torch.where(r > 0, ref, zero)
        assert ref.dtype == torch.float32
        assert _same_bits(g, ref), tag
        assert not bool(torch.isnan(g).any()), tag
        if with_r or with_sc:
            assert g.data_ptr() == gout.data_ptr() and bool(torch.isnan(gbuf[:, :4]).all()) and bool(torch.isnan(gbuf[:, 4 + N:]).all()), tag   # the pads untouched
        else:
            assert g is dyd and bool(torch.isnan(dybuf[:, N:]).all()) and not bool(gout.any()), tag             # nothing to write: g is dy itself
        terms = [ref.double(), dy.double(), dy.double() * r.double() if with_r else torch.zeros(M, N, dtype=torch.float64)]
        for j, (name, t) in enumerate(zip(("sum g", "sum dy", "sum dy * r"), terms)):
            ours, want = sums[j].cpu(), t.sum(0)
            nan_cols = torch.isnan(want)                                    # the column of the planted NaN (sum dy * r only): NaN on both sides
            assert bool(torch.isnan(ours[nan_cols]).all()) and (j == 2 or not bool(nan_cols.any())), (tag, name)
            err = (ours - want).abs()[~nan_cols]
            bound = (M * 2.0 ** -52 * t.abs().sum(0))[~nan_cols]
            ratio = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
            print(f"[grad-error] {tag} {name}: largest error {float(err.max()) if err.numel() else 0.0:.3e}, largest error / bound {ratio:.3e}")
            assert bool((err <= bound).all()), (tag, name)
        g2, sums2 = run()
        assert _same_bits(g2, g) and torch.equal(sums2.cpu().view(torch.int64), sums.cpu().view(torch.int64)), tag


# ------------------------------------------------------------------------------------------------ 2. gn_linear_bwd_weight, directly
# (M, N, K, (ld, offset) of g, (ld, offset) of x, (ld, offset) of dW) -- None: rows of exactly that many floats
WEIGHT_CASES = {
    "1-1-1": (1, 1, 1, None, None, None),                                  # rows of exactly C floats: the scalar path
    "7-3-5": (7, 3, 5, None, None, None),
    "65-33-31": (65, 33, 31, (36, 0), (32, 0), None),                       # an odd last row pair, one column past a 32-tile each way; float4 path, its tails
    "R+1-128-131": (R + 1, 128, 131, None, (132, 0), None),                 # one row in the second chunk; the odd production width
    "2R+7-1-256": (2 * R + 7, 1, 256, (4, 0), None, None),                  # the decoder heads
    "2R+7-3-256": (2 * R + 7, 3, 256, (4, 0), None, None),
    "3R-1-257-64": (3 * R - 1, 257, 64, (270, 3), (77, 5), (70, 2)),         # column slices of wider NaN-filled buffers, each at its own offset and stride
    "130-1024-1280": (130, 1024, 1280, None, None, None),                   # many blocks, few rows
    "4R-128-32": (4 * R, 128, 32, None, None, None),                        # the 128 x 32 variant (K <= 32), whole chunks
    # the UNet's final 1x1x1 convolution (autograd.unet3d hands it to this kernel: K = the stored input channels)
    "1031-8-32-ldx40": (1031, 8, 32, None, (40, 0), None),                  # x 40 columns wide (ldx > K); a 7-row third chunk
    "2061-128-32": (2061, 128, 32, None, None, None),                       # the production N x K, the K <= 32 variant over five chunks, the last of 13 rows
    "300-512-7": (300, 512, 7, None, None, None),
    "520-5-1023": (520, 5, 1023, (8, 0), (1024, 0), None),                  # K % 4 = 3 in rows of 1024: the float4 loader's scalar tail, a partial last K block
}


@pytest.mark.parametrize("case", list(WEIGHT_CASES))
def test_linear_bwd_weight_direct(case):
    M, N, K, gl, xl, wl = WEIGHT_CASES[case]
    g_ = _gen(sum(map(ord, case)))
    g = torch.randn(M, N, generator=g_)
    x = torch.randn(M, K, generator=g_) + 0.25
    gd = g.to(DEV) if gl is None else _embed(g, *gl)[0]
    xd = x.to(DEV) if xl is None else _embed(x, *xl)[0]
    out, obuf = (None, None) if wl is None else _embed(torch.zeros(N, K), *wl)
    dw = ops.linear_bwd_weight(gd, xd, out=out)
    assert tuple(dw.shape) == (N, K) and not bool(torch.isnan(dw).any()), case           # no NaN leaks from the padding
    if wl is not None:
        assert bool(torch.isnan(obuf[:, :wl[1]]).all()) and bool(torch.isnan(obuf[:, wl[1] + K:]).all()), case
    ref64 = g.double().t() @ x.double()
    derived = (R + 2) * 2.0 ** -24 * (g.abs().double().t() @ x.abs().double())
    err = (dw.double().cpu() - ref64).abs()
    print(f"[grad-error] linear_bwd_weight {case}: largest error / derived bound {float((err / derived).max()):.3e}")
    _check(f"linear_bwd_weight {case}", ref64, g.t() @ x, dw)
    assert bool((err <= derived).all()), case
    assert _same_bits(ops.linear_bwd_weight(gd, xd), dw), case


def test_linear_bwd_weight_of_no_rows_is_exact_zeros():
    dw = ops.linear_bwd_weight(torch.empty(0, 6, device=DEV), torch.empty(0, 9, device=DEV))
    assert tuple(dw.shape) == (6, 9) and not bool(_bits(dw).any())


def test_row_affine_is_the_fused_epilogue_bit_for_bit():
    """ops.row_affine(relu(x W^T + b)) against gn_linear's own BatchNorm epilogue, at a width and a row count that are no multiple of anything"""
    g_ = _gen(9)
    x, w, b = torch.randn(301, 37, generator=g_).to(DEV), torch.randn(131, 40, generator=g_).to(DEV), torch.randn(131, generator=g_).to(DEV)
    sc, sh = torch.randn(131, generator=g_).to(DEV), torch.randn(131, generator=g_).to(DEV)
    fused = ops.linear(x, w, b, sc, sh, relu=True, K=37)
    assert _same_bits(ops.row_affine(ops.linear(x, w, b, None, None, relu=True, K=37), sc, sh), fused)


# ------------------------------------------------------------------------------------------------ restatement (plain torch, any dtype, CPU)
def r_block(x, w, b, bn, mask=None):
    """F.linear -> relu (or the shared mask) -> eval F.batch_norm.  bn: (running_mean, running_var, gamma, beta, eps) or None"""
    h = F.linear(x, w, b)
    r = F.relu(h) if mask is None else h * mask
    return r if bn is None else F.batch_norm(r, bn[0], bn[1], bn[2], bn[3], False, 0.0, bn[4])


def r_mlp(stack, P, h, masks=None, prefix=""):
    """stack: the CPU module (structure, running statistics); P: its parameters in h's dtype"""
    for i, block in enumerate(stack):
        bn = block[2] if len(block) > 2 else None
        bnp = None if bn is None else (bn.running_mean.to(h.dtype), bn.running_var.to(h.dtype), P[f"{prefix}{i}.2.weight"], P[f"{prefix}{i}.2.bias"], bn.eps)
        h = r_block(h, P[f"{prefix}{i}.0.weight"], P[f"{prefix}{i}.0.bias"], bnp, None if masks is None else masks[i].to(h.dtype))
    return h


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def _params(module, dtype, prefix=""):
    return {prefix + k: p.detach().to(dtype).requires_grad_(True) for k, p in module.named_parameters()}


def _stack(channels, seed, batch_norm=True):
    torch.manual_seed(seed)
    stack = MLP(channels, batch_norm=batch_norm)
    _randomise_norms(stack, _gen(seed + 1000))
    return stack.eval()


def hip_masks(stack_gpu, rows):
    """the r > 0 of every block of the HIP forward on `rows` (the kernels autograd.mlp runs), and the forward's result"""
    masks, h = [], rows
    with torch.no_grad():
        for wp, b, sc, sh, k in stack_gpu.packed():
            r = ops.linear(h, wp, b, None, None, relu=True, K=k)
            masks.append((r > 0).cpu())
            h = r if sc is None else ops.row_affine(r, sc, sh)
    return masks, h


def restated_mlp_grads(stack, x, dy, dtype, masks):
    P = _params(stack, dtype)
    xx = _leaf(x, dtype)
    y = r_mlp(stack, P, xx.reshape(-1, x.shape[-1]), masks).reshape(*x.shape[:-1], -1)
    return dict(zip(["x"] + list(P), torch.autograd.grad(y, [xx] + list(P.values()), dy.to(dtype))))


def hip_mlp_grads(stack_gpu, x, dy, x_grad=True):
    xg = x.to(DEV).requires_grad_(x_grad)
    y = A.mlp(stack_gpu, xg)
    names = (["x"] if x_grad else []) + [k for k, _ in stack_gpu.named_parameters()]
    return y.detach(), dict(zip(names, torch.autograd.grad(y, ([xg] if x_grad else []) + list(stack_gpu.parameters()), dy.to(DEV))))


def _compare(tag, g64, g32, gh):
    assert set(gh) == set(g64), (tag, sorted(gh), sorted(g64))
    return max(_check(f"{tag} d {k}", g64[k], g32[k], gh[k]) for k in g64)


# ------------------------------------------------------------------------------------------------ 3. block and stack gradients
STACKS = {"sa1": ([6, 64, 64, 128], 1000, True), "sa2": ([131, 128, 128, 256], 700, True), "agg": ([137, 137, 128], 900, True),
          "dec1": ([128, 256, 256, 1], 1100, True), "dec3": ([128, 256, 256, 3], 1100, True), "no_bn": ([20, 48, 32], 600, False)}


@pytest.mark.parametrize("which", list(STACKS))
def test_stack_gradients(which):
    channels, rows, bn = STACKS[which]
    seed = sum(map(ord, which))
    stack = _stack(channels, seed, bn)
    sg = copy.deepcopy(stack).to(DEV)
    g_ = _gen(seed + 1)
    x = torch.randn(rows, channels[0], generator=g_)
    dy = torch.randn(rows, channels[-1], generator=g_)
    masks, fwd = hip_masks(sg, x.to(DEV))
    with torch.no_grad():
        plain = sg(x.to(DEV))
    assert _same_bits(fwd, plain), which
    y, gh = hip_mlp_grads(sg, x, dy)
    assert _same_bits(y, plain), which                                      # the forward bits are stack(x)'s in grad mode ...
    with torch.no_grad():
        assert _same_bits(A.mlp(sg, x.to(DEV)), plain), which              # ... and under no_grad
    g64, g32 = (restated_mlp_grads(stack, x, dy, dt, masks) for dt in (torch.float64, torch.float32))
    _compare(f"stack {which}", g64, g32, gh)
    # two runs, every tensor bit for bit
    y2, gh2 = hip_mlp_grads(sg, x, dy)
    assert _same_bits(y2, y) and all(_same_bits(gh2[k], gh[k]) for k in gh), which
    # leading dimensions (B, M, C)
    y3, gh3 = hip_mlp_grads(sg, x.view(2, rows // 2, -1), dy.view(2, rows // 2, -1))
    assert tuple(y3.shape) == (2, rows // 2, channels[-1]) and _same_bits(y3.reshape(rows, -1), y), which
    assert tuple(gh3["x"].shape) == (2, rows // 2, channels[0]) and all(_same_bits(gh3[k].reshape(gh[k].shape), gh[k]) for k in gh), which
    # an x that needs no gradient: no dX launch for the first block (its transposed pack is never built; the later blocks' inputs do need theirs),
    # the parameter gradients unchanged
    fresh = copy.deepcopy(stack).to(DEV)
    _, gp = hip_mlp_grads(fresh, x, dy, x_grad=False)
    assert "x" not in gp and all(_same_bits(gp[k], gh[k]) for k in gp), which
    assert set(param_cache(fresh, "_grad_packs")._items) == {("wt", i) for i in range(1, len(channels) - 1)}, which
    assert set(param_cache(sg, "_grad_packs")._items) == {("wt", i) for i in range(len(channels) - 1)}, which


def test_an_in_place_parameter_update_between_forward_and_backward_raises():
    sg = _stack([6, 16, 8], 3).to(DEV)
    y = A.mlp(sg, torch.randn(50, 6, generator=_gen(4)).to(DEV).requires_grad_(True))
    with torch.no_grad():
        sg[1][0].weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()
    # the next forward runs on the updated parameters (its packs are keyed by the parameters' versions)
    x = torch.randn(50, 6, generator=_gen(5)).to(DEV)
    ref = copy.deepcopy(sg)
    with torch.no_grad():
        want = ref(x)
    assert _same_bits(A.mlp(sg, x.clone().requires_grad_(True)), want)


# ------------------------------------------------------------------------------------------------ 4. A.linear
@pytest.mark.parametrize("cin,cout,rows,relu", [(128, 128, 500, True), (128, 128, 500, False), (1024, 1024, 8, False)])
def test_hip_linear_gradients(cin, cout, rows, relu):
    torch.manual_seed(cin + rows + relu)
    lin = HipLinear(cin, cout)
    lg = copy.deepcopy(lin).to(DEV)
    g_ = _gen(cin + 7 * rows + relu)
    x, dy = torch.randn(rows, cin, generator=g_), torch.randn(rows, cout, generator=g_)
    with torch.no_grad():
        plain = lg(x.to(DEV), relu=relu)
    mask = (plain > 0).cpu() if relu else None

    def hip():
        xg = x.to(DEV).requires_grad_(True)
        y = A.linear(lg, xg, relu=relu)
        return y.detach(), dict(zip(("x", "weight", "bias"), torch.autograd.grad(y, [xg, lg.weight, lg.bias], dy.to(DEV))))
    y, gh = hip()
    assert _same_bits(y, plain)
    with torch.no_grad():
        assert _same_bits(A.linear(lg, x.to(DEV), relu=relu), plain)
    res = {}
    for dt in (torch.float64, torch.float32):
        P = _params(lin, dt)
        xx = _leaf(x, dt)
        h = F.linear(xx, P["weight"], P["bias"])
        out = h * mask.to(dt) if relu else h
        res[dt] = dict(zip(("x", "weight", "bias"), torch.autograd.grad(out, [xx, P["weight"], P["bias"]], dy.to(dt))))
    _compare(f"linear {cin}->{cout} rows={rows} relu={relu}", res[torch.float64], res[torch.float32], gh)
    y2, gh2 = hip()
    assert _same_bits(y2, y) and all(_same_bits(gh2[k], gh[k]) for k in gh)


# ------------------------------------------------------------------------------------------------ 5. compositions
def test_point_conv_max_through_a_differentiable_stack():
    """PointConv(local_nn = autograd.mlp(stack), aggr='max') on 2 x 256 points, K = 16: gradients to the features and to the stack's parameters.  The
    ReLU masks of the stack are the HIP forward's; the max winners are each side's own (tests/test_gpu_autograd.py's way)."""
    sizes, C, K = [256, 256], 13, 16
    n = sum(sizes)
    g_ = _gen(31)
    pos, x = torch.rand(n, 3, generator=g_), torch.randn(n, C, generator=g_)
    stack = _stack([C + 3, 32, 24], 32)
    sg = copy.deepcopy(stack).to(DEV)
    pd = pos.to(DEV)
    seg0 = Segments(sizes, DEV)
    idx = A.fps(pd, seg0, 0.5)
    seg1 = Segments([ops.fps_count(s, 0.5) for s in sizes], DEV)
    nbr, _ = A.ball_table(pd, idx, 0.25, seg0, seg1, K)
    Mc, S = nbr.shape[0], K + 1
    with torch.no_grad():
        edges, slot, _ = ops.sa_gather(x.to(DEV), pd, idx.to(torch.int32), nbr)
    masks, _ = hip_masks(sg, edges)
    slot = slot.cpu()
    dy = torch.randn(Mc, 24, generator=g_)

    def hip():
        xg = x.to(DEV).requires_grad_(True)
        out = A.point_conv_max(xg, pd, idx, nbr, lambda e: A.mlp(sg, e))
        return dict(zip(["x"] + [k for k, _ in sg.named_parameters()], torch.autograd.grad(out, [xg] + list(sg.parameters()), dy.to(DEV))))
    res = {}
    for dt in (torch.float64, torch.float32):
        P = _params(stack, dt)
        xx = _leaf(x, dt)
        out = r_segment_max(r_mlp(stack, P, r_sa_gather(xx, pos.to(dt), idx.cpu(), slot, S), masks), slot, Mc, S)
        res[dt] = dict(zip(["x"] + list(P), torch.autograd.grad(out, [xx] + list(P.values()), dy.to(dt))))
    gh = hip()
    _compare("point_conv_max(mlp)", res[torch.float64], res[torch.float32], gh)
    gh2 = hip()
    assert all(_same_bits(gh2[k], gh[k]) for k in gh)


def test_implicit_decode_gradients():
    """autograd.implicit_decode alone: gradient to the volume, the queries (drawn in [-0.1, 1.1]: some clamp at the border) and the decoder's parameters"""
    g_ = _gen(41)
    B, C, dims, Mq = 2, 8, (6, 7, 5), 400
    torch.manual_seed(42)
    dec = ImplicitWNFDecoder(nn_channels=(C, 64, 64, 1))
    _randomise_norms(dec, _gen(43))
    dec.eval()
    dg = copy.deepcopy(dec).to(DEV)
    vol = torch.randn(B, C, *dims, generator=g_)
    q = torch.rand(B, Mq, 3, generator=g_) * 1.2 - 0.1
    dy = torch.randn(B, Mq, 1, generator=g_)
    with torch.no_grad():
        rows = A.grid_sample_points(vol.to(DEV), q.to(DEV))
        masks, _ = hip_masks(dg.mlp, rows.reshape(-1, C))

    def hip():
        vg, qg = vol.to(DEV).requires_grad_(True), q.to(DEV).requires_grad_(True)
        y = A.implicit_decode(dg, vg, qg)
        assert tuple(y.shape) == (B, Mq, 1)
        return dict(zip(["volume", "query"] + ["mlp." + k for k, _ in dg.mlp.named_parameters()], torch.autograd.grad(y, [vg, qg] + list(dg.mlp.parameters()), dy.to(DEV))))
    res = {}
    for dt in (torch.float64, torch.float32):
        P = _params(dec.mlp, dt, "mlp.")
        vv, qq = _leaf(vol, dt), _leaf(q, dt)
        y = r_mlp(dec.mlp, P, r_sample(vv, qq).reshape(-1, C), masks, "mlp.").reshape(B, Mq, 1)
        res[dt] = dict(zip(["volume", "query"] + list(P), torch.autograd.grad(y, [vv, qq] + list(P.values()), dy.to(dt))))
    gh = hip()
    _compare("implicit_decode", res[torch.float64], res[torch.float32], gh)
    gh2 = hip()
    assert all(_same_bits(gh2[k], gh[k]) for k in gh)


def test_second_stage_gradient_to_the_rows_and_every_parameter():
    """rows (2 * 600, 20) -> autograd.mlp(MLP([20, 48, 32])) -> autograd.scatter (mean) into 16^3 -> autograd.unet3d (f_maps (32, 64), strict-fp32 forward)
    -> autograd.implicit_decode (nn_channels (8, 64, 64, 1)) -> F.mse_loss: gradients to the input rows and to EVERY parameter of the three modules
    (tests/test_gpu_unet_grad.py::test_second_stage_chain_gradient's setup, extended at both ends).  Each side forms its own masks and pool winners."""
    def r_scatter_mean(src, cell, cells):
        mask = (cell[None, :] == torch.arange(cells)[:, None]).to(src.dtype)
        return (mask @ src) / mask.sum(1).clamp(min=1)[:, None]
    g_ = _gen(61)
    B, n, C0, C, G, Mq, CO = 2, 600, 20, 32, 16, 300, 8
    agg = _stack([C0, 48, C], 71)
    torch.manual_seed(11)
    unet = Abstract3DUNet(C, CO, f_maps=(32, 64), num_groups=8)
    _randomise_norms(unet, g_)
    torch.manual_seed(72)
    dec = ImplicitWNFDecoder(nn_channels=(CO, 64, 64, 1))
    _randomise_norms(dec, _gen(73))
    dec.eval()
    rows = torch.randn(B * n, C0, generator=g_)
    cell = torch.randint(0, G, (B * n, 3), generator=g_)
    cell[:200] = cell[0]
    batch = torch.arange(B).repeat_interleave(n)
    flat = ((batch * G + cell[:, 0]) * G + cell[:, 1]) * G + cell[:, 2]
    q = torch.rand(B, Mq, 3, generator=g_) * 1.2 - 0.1
    tgt = torch.randn(B, Mq, 1, generator=g_)
    res = {}
    for dt in (torch.float64, torch.float32):
        P = {**_params(agg, dt, "agg."), **_params(unet, dt, "unet."), **_params(dec.mlp, dt, "dec.")}
        rr = _leaf(rows, dt)
        f = r_mlp(agg, P, rr, None, "agg.")
        vol = r_scatter_mean(f, flat, B * G ** 3).view(B, G, G, G, C).permute(0, 4, 1, 2, 3)
        pred = r_mlp(dec.mlp, P, r_sample(r_unet(unet, P, vol, prefix="unet."), q.to(dt)).reshape(-1, CO), None, "dec.").reshape(B, Mq, 1)
        loss = F.mse_loss(pred, tgt.to(dt))
        res[dt] = (float(loss.detach()), dict(zip(["rows"] + list(P), torch.autograd.grad(loss, [rr] + list(P.values())))))
    ag, ug, dg = (copy.deepcopy(m).to(DEV) for m in (agg, unet, dec))
    named = [("agg." + k, p) for k, p in ag.named_parameters()] + [("unet." + k, p) for k, p in ug.named_parameters()] + \
            [("dec." + k, p) for k, p in dg.mlp.named_parameters()]

    def hip():
        rr = rows.to(DEV).requires_grad_(True)
        f = A.mlp(ag, rr)
        vol = A.scatter(f.t(), flat.to(DEV), -1, B * G ** 3, "mean").view(C, B, G, G, G).permute(1, 0, 2, 3, 4)
        pred = A.implicit_decode(dg, A.unet3d(ug, vol, arith=AR.DEFAULT.strict_fp32()), q.to(DEV))
        loss = F.mse_loss(pred, tgt.to(DEV))
        return float(loss.detach()), dict(zip(["rows"] + [k for k, _ in named], torch.autograd.grad(loss, [rr] + [p for _, p in named])))
    lh, gh = hip()
    l64 = res[torch.float64][0]
    print(f"[grad-error] second stage loss: fp64 {l64:.9e}  hip {lh:.9e}  relative {abs(lh - l64) / abs(l64):.3e}")
    assert abs(lh - l64) <= 1e-5 * abs(l64)
    _compare("second stage", res[torch.float64][1], res[torch.float32][1], gh)
    lh2, gh2 = hip()
    assert lh2 == lh and all(_same_bits(gh2[k], gh[k]) for k in gh)


# ------------------------------------------------------------------------------------------------ 6. production shapes, once each
@pytest.mark.parametrize("rows,cin,cout", [(144000, 128, 256), (48000, 137, 137)])
def test_production_shape(rows, cin, cout):
    """the decoder's first layer and the aggregator's layer at the reference's validation row counts, one block each: the rule, and bit equality"""
    stack = _stack([cin, cout], rows % 1000 + cin)
    sg = copy.deepcopy(stack).to(DEV)
    g_ = _gen(rows + cin)
    x, dy = torch.randn(rows, cin, generator=g_), torch.randn(rows, cout, generator=g_)
    masks, _ = hip_masks(sg, x.to(DEV))
    y, gh = hip_mlp_grads(sg, x, dy)
    g64, g32 = (restated_mlp_grads(stack, x, dy, dt, masks) for dt in (torch.float64, torch.float32))
    _compare(f"production {rows} x {cin} -> {cout}", g64, g32, gh)
    y2, gh2 = hip_mlp_grads(sg, x, dy)
    assert _same_bits(y2, y) and all(_same_bits(gh2[k], gh[k]) for k in gh)
