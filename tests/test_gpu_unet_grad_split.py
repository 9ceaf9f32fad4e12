"""GPU (-m gpu): the f16x2 backward of the UNet convolutions (arith.Arith.conv_grad_mode = "f16x2": csrc/unet_grad_split.hip, the data gradient on
csrc/unet_split.hip's direct kernels; autograd._conv_gcr_backward_split).

Rule: grad_reference._check, unchanged -- ours against fp64 at most K_F16X2_BWD x (torch-fp32 against fp64) + 1 fp32 ulp of the largest gradient, every
element finite, every figure printed as `[grad-error] ...` before it is asserted.  The references are tests/test_gpu_unet_grad.py's (its restatements,
shapes and inputs, imported): the layer cases are handed the ReLU mask of the HIP forward, the compositions the HIP forward's masks and pool winners.
The forward is strict fp32 wherever the backward is measured, so only the backward moves.

K_F16X2_BWD: set as K_F16X2 of tests/test_gpu_unet_grad.py was -- one run with every ratio printed, the largest rounded up to the next power of two.
An f16x2 operand carries about 2^-22 relative error against fp32's 2^-24, so a ratio above 8 would not be rounding and is not adopted.
Measured on an MI355X (largest ratio ours / torch-fp32 per group of tests):
    one layer, the ten shapes:             1.57  1.80  1.42  1.66  1.64 (cubic)   1.99  2.21  1.11  1.41  1.86 (ragged)
    the weight-gradient kernel directly:   0.17 (chains, masked)  0.13 (chains, y = None)  0.90 (c20+12)
    scales: 2^-20 / 1 / 2^20 direct 0.39, through the layer 1.34 (the small sample's d src0 alone 0.91); dy x 1e30 0.96 / 1.77, x 1e-30 0.98 / 1.30
            (direct / layer); 1e-30 .. 1e30 inside every sample 1.94
    compositions, shared selections:       2.16 (main)  1.20 (padded_4x12x10)  1.59 (main_4x8x12)
    a training step, 52 tensors:           0.13 - 2.41 (the largest is surface_decoder.mlp.2.2.bias, a tensor behind no convolution: the fp32 backward's
                                           own figure in tests/test_gpu_train_pipeline.py; the UNet's tensors 0.34 - 0.93)
The largest is 2.41 (2.21 on a convolution's own gradients): K_F16X2_BWD = 4.

Which case reaches what of csrc/unet_grad_split.hip: the NCO = 1 kernel: the 32- and 96-wide outputs; ragged tiles in z, y, x (the zero fills of both
stagings, every transposed read still inside the images): the LAYER_RAGGED cases; a 32-block holding both sources and half beyond Cin: 16+32; a chain
spanning two samples (the per-sample multiplier switches in mid-chain) and a one-tile last chain: [chains-*]; source 1 from channel 20: [c20+12].
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from garmentnets_amd import _lib, arith as AR, autograd as A, ops  # noqa: E402
from garmentnets_amd.components import unet3d as U  # noqa: E402
from garmentnets_amd.components.unet3d import SingleConv, stored_channels  # noqa: E402
from grad_reference import _check, _gen, _randomise_norms, r_layer  # noqa: E402
from test_gpu_unet_grad import (BW_DIRECT, COMPOSITIONS, LAYER_CUBIC, LAYER_RAGGED, _cl, _compare_all, _composition_inputs, _to_stored_cl,  # noqa: E402
                                hip_selections, hip_unet_grads, restated_unet_grads)

DEV = "cuda:0"
K_F16X2_BWD = 4        # the measured ratios (module docstring: at most 2.41) rounded up to the next power of two
FP32 = AR.DEFAULT.strict_fp32()
SPLIT = FP32.replace(conv_grad_mode="f16x2")            # strict-fp32 forward, f16x2 backward


class _Spy:
    """counts the calls of the two f16x2 gradient entries (and of their fp32 counterparts) made while it is active: a silent fallback cannot pass"""
    NAMES = ("conv3d_bwd_weight_split", "conv3d_bwd_data_split", "conv3d_bwd_weight", "conv3d_bwd_data")

    def __init__(self, monkeypatch):
        self.calls = {n: 0 for n in self.NAMES}
        for n in self.NAMES:
            monkeypatch.setattr(ops, n, self._wrap(n, getattr(ops, n)))

    def _wrap(self, name, fn):
        def wrapped(*a, **kw):
            self.calls[name] += 1
            return fn(*a, **kw)
        return wrapped


# ------------------------------------------------------------------------------------------------ 1. one layer
def _layer_case(real, stored, cout, dims, B, r_scale=None):
    """the inputs of test_gpu_unet_grad.test_layer_gradients; r_scale [B]: a per-sample factor on the output gradient"""
    g = _gen(sum(real) + cout)
    conv = SingleConv(sum(real), cout)
    conv.in_real = real
    _randomise_norms(conv, g)
    x0 = torch.randn(B, real[0], *dims, generator=g) * 1.5 + 0.3
    x1 = torch.randn(B, real[1], *(n // 2 for n in dims), generator=g) if len(real) > 1 else None
    R = torch.randn(B, cout, *dims, generator=g)
    if r_scale is not None:
        R = R * torch.as_tensor(r_scale, dtype=torch.float32).view(B, 1, 1, 1, 1)
    return conv, x0, x1, R


def _hip_layer(conv, x0, x1, R, stored, arith):
    """-> (y, [d src0, (d src1,) d weight, d gamma, d beta]) of A.conv3d_gcr under the output gradient R"""
    cout, cs = conv.conv.out_channels, stored_channels(conv.conv.out_channels)
    cg = copy.deepcopy(conv).to(DEV)
    s0 = _to_stored_cl(x0, stored[0]).to(DEV).requires_grad_(True)
    s1 = None if x1 is None else _to_stored_cl(x1, stored[1]).to(DEV).requires_grad_(True)
    y = A.conv3d_gcr(cg, s0, s1, arith=arith)
    assert y.grad_fn is not None and not bool(y[..., cout:].any())
    leaves = [s0] + ([s1] if s1 is not None else []) + [cg.conv.weight, cg.groupnorm.weight, cg.groupnorm.bias]
    return y.detach(), list(torch.autograd.grad(y, leaves, _to_stored_cl(R, cs).to(DEV)))


def _restated_layer(conv, x0, x1, R, mask):
    res = {}
    for dtype in (torch.float64, torch.float32):
        lv = [t.detach().to(dtype).requires_grad_(True) for t in [x0] + ([x1] if x1 is not None else []) + [conv.conv.weight, conv.groupnorm.weight, conv.groupnorm.bias]]
        out = r_layer(lv[0], lv[1] if x1 is not None else None, lv[-3], lv[-2], lv[-1], conv.groupnorm.num_groups, conv.groupnorm.eps, mask=mask.to(dtype))
        res[dtype] = torch.autograd.grad(out, lv, R.to(dtype))
    return res


def _check_layer(tag, conv, x0, x1, R, real, stored, monkeypatch):
    """every gradient of one layer under SPLIT held to the rule, the pads exact zeros, both f16x2 kernels seen running -> the ratios"""
    cout, dims = conv.conv.out_channels, tuple(x0.shape[2:])
    plan = U.conv_grad_plan(SPLIT, dims, stored[0], stored[1] if len(stored) > 1 else 0, stored_channels(cout))
    assert plan == U.ConvGradPlan("f16x2", "f16x2")
    spy = _Spy(monkeypatch)
    y, gh = _hip_layer(conv, x0, x1, R, stored, SPLIT)
    assert spy.calls == {"conv3d_bwd_weight_split": 1, "conv3d_bwd_data_split": 1, "conv3d_bwd_weight": 0, "conv3d_bwd_data": 0}, spy.calls
    mask = (y[..., :cout] > 0).permute(0, 4, 1, 2, 3).cpu()
    res = _restated_layer(conv, x0, x1, R, mask)
    names = ["d src0"] + (["d src1"] if x1 is not None else []) + ["d weight", "d gamma", "d beta"]
    ratios = []
    for i, name in enumerate(names):
        ours = gh[i]
        if name.startswith("d src"):
            r = real[int(name[-1])]
            assert not bool(ours[..., r:].any()), f"{name}: pad gradients must be exact zeros"
            ours = ours[..., :r].permute(0, 4, 1, 2, 3)
        ratios.append(_check(f"split {tag} {name}", res[torch.float64][i], res[torch.float32][i], ours, K_F16X2_BWD))
    print(f"[grad-error] split {tag}: largest ratio to e32 {max(ratios):.2f}")
    return ratios


@pytest.mark.parametrize("real,stored,cout,dims,B",
                         [pytest.param(*c, 2, id="{}to{}-{}-B2".format("+".join(map(str, c[0])), c[2], "x".join(map(str, c[3])))) for c in LAYER_CUBIC]
                         + [pytest.param(*c, id="{}to{}-{}-B{}".format("+".join(map(str, c[0])), c[2], "x".join(map(str, c[3])), c[4])) for c in LAYER_RAGGED])
def test_layer_gradients_split(real, stored, cout, dims, B, monkeypatch):
    conv, x0, x1, R = _layer_case(real, stored, cout, dims, B)
    _check_layer(f"layer {real}->{cout} {dims} B={B}", conv, x0, x1, R, real, stored, monkeypatch)


# ------------------------------------------------------------------------------------------------ 2. the weight-gradient kernel called directly
def _direct_case(case, dy_scale=None):
    c = BW_DIRECT[case]
    B, dims, C0, C1, cout = c["B"], c["dims"], c["C0"], c["C1"], c["cout"]
    g = _gen(C0 + C1 + cout)
    x0 = torch.randn(B, C0, *dims, generator=g)
    x1 = torch.randn(B, C1, *(n // 2 for n in dims), generator=g) if C1 else None
    a = 0.5 + torch.rand(B, C0 + C1, generator=g)
    d = 0.3 * torch.randn(B, C0 + C1, generator=g)
    y = torch.randn(B, cout, *dims, generator=g)
    y[:, :, 0, 0, ::2] = 0.0
    y[:, :, 1, 1, ::2] = -0.0
    dy = torch.randn(B, cout, *dims, generator=g)
    if dy_scale is not None:
        dy = dy * dy_scale
    return x0, x1, a, d, y, dy


def _direct_reference(x0, x1, a, d, y, dy, masked):
    res = {}
    cout, cin = dy.shape[1], a.shape[1]
    for dtype in (torch.float64, torch.float32):
        x = x0.to(dtype) if x1 is None else torch.cat((x0.to(dtype), F.interpolate(x1.to(dtype), scale_factor=2, mode="nearest")), 1)
        w = torch.zeros(cout, cin, 3, 3, 3, dtype=dtype, requires_grad=True)
        out = F.conv3d(x * a.to(dtype)[:, :, None, None, None] + d.to(dtype)[:, :, None, None, None], w, padding=1)
        (res[dtype],) = torch.autograd.grad(out, w, (dy * (y > 0) if masked else dy).to(dtype))
    return res


def _direct_args(x0, x1, a, d, y, dy, masked):
    return (_cl(x0).to(DEV), None if x1 is None else _cl(x1).to(DEV), a.to(DEV), d.to(DEV), _cl(y).to(DEV) if masked else None, _cl(dy).to(DEV))


@pytest.mark.parametrize("case,masked", [("chains", True), ("chains", False), ("c20+12", True)])
def test_conv3d_bwd_weight_split_direct(case, masked):
    """ops.conv3d_bwd_weight_split against d/dw of conv3d(x * a + d, w, padding=1) under dy (masked by y > 0, or y = None): the inputs of
    test_conv3d_bwd_weight_direct.  chains: 15 tiles, 48 blocks -> 8 chains of 2 (chain 2 spans samples 0 / 1, chain 7 holds one tile), asserted on the
    host from the workspace size.  c20+12: widths on the far side of the plan's quad rule's neighbours (multiples of 4, no multiple of 16)"""
    c = BW_DIRECT[case]
    if case == "chains":
        lib = _lib.load()
        header = -(-(16 + 4 * c["B"]) // 256) * 256
        assert lib.gn_conv3d_bwd_weight_split_workspace_bytes(c["B"], *c["dims"], c["C0"] + c["C1"], c["cout"]) == header + 8 * 27 * 384 * 256 * 4
        assert lib.gn_conv3d_bwd_weight_workspace_bytes(c["B"], *c["dims"], c["C0"] + c["C1"], c["cout"]) == 8 * 27 * 384 * 256 * 4
    else:
        assert U.conv_grad_plan(SPLIT, c["dims"], c["C0"], c["C1"], c["cout"]).weight == "f16x2"
        assert U.conv_grad_plan(SPLIT, c["dims"], c["C0"] + 2, c["C1"], c["cout"]).weight == "fp32"
    inputs = _direct_case(case)
    res = _direct_reference(*inputs, masked)
    args = _direct_args(*inputs, masked)
    ours = ops.conv3d_bwd_weight_split(*args)
    _check(f"conv3d_bwd_weight_split {case} {'masked' if masked else 'y=None'} d weight", res[torch.float64], res[torch.float32], ours, K_F16X2_BWD)
    assert torch.equal(ours, ops.conv3d_bwd_weight_split(*args))


# ------------------------------------------------------------------------------------------------ 3. scales
SCALE_LAYER = ((32, 64), (32, 64), 64, (8, 8, 8), 2)


def test_all_zero_dy_gives_exact_zeros(monkeypatch):
    x0, x1, a, d, y, dy = _direct_case("c20+12")
    dw = ops.conv3d_bwd_weight_split(*_direct_args(x0, x1, a, d, y, torch.zeros_like(dy), True))
    assert not bool(dw.any()) and bool(torch.isfinite(dw).all())
    real, stored, cout, dims, B = SCALE_LAYER
    conv, x0, x1, R = _layer_case(real, stored, cout, dims, B)
    spy = _Spy(monkeypatch)
    _, gh = _hip_layer(conv, x0, x1, torch.zeros_like(R), stored, SPLIT)
    assert spy.calls["conv3d_bwd_weight_split"] == 1 and spy.calls["conv3d_bwd_data_split"] == 1
    for t in gh[:3]:                       # d src0, d src1, d weight: exact zeros (no 0 * inf)
        assert not bool(t.any()) and bool(torch.isfinite(t).all())
    for t in gh[3:]:
        assert bool(torch.isfinite(t).all()) and not bool(t.any())


def test_samples_of_very_different_gradient_scale(monkeypatch):
    """one sample's dy times 2^-20, another's times 2^20: the data gradient scales per sample, the weight gradient per launch -- both inside the rule"""
    x0, x1, a, d, y, dy = _direct_case("chains", torch.tensor([2.0 ** -20, 1.0, 2.0 ** 20]).view(3, 1, 1, 1, 1))
    res = _direct_reference(x0, x1, a, d, y, dy, True)
    ours = ops.conv3d_bwd_weight_split(*_direct_args(x0, x1, a, d, y, dy, True))
    _check("split scales 2^-20 / 1 / 2^20 direct d weight", res[torch.float64], res[torch.float32], ours, K_F16X2_BWD)
    real, stored, cout, dims, B = SCALE_LAYER
    conv, x0, x1, R = _layer_case(real, stored, cout, dims, B, r_scale=[2.0 ** -20, 2.0 ** 20])
    _check_layer("scales 2^-20 / 2^20 layer", conv, x0, x1, R, real, stored, monkeypatch)
    # the small sample keeps its own precision in d src: held to the rule on its own
    conv, x0, x1, R = _layer_case(real, stored, cout, dims, B, r_scale=[2.0 ** -20, 2.0 ** 20])
    y, gh = _hip_layer(conv, x0, x1, R, stored, SPLIT)
    res = _restated_layer(conv, x0, x1, R, (y[..., :cout] > 0).permute(0, 4, 1, 2, 3).cpu())
    _check("scales 2^-20 / 2^20 layer d src0, the small sample alone", res[torch.float64][0][:1], res[torch.float32][0][:1], gh[0][:1].permute(0, 4, 1, 2, 3),
           K_F16X2_BWD)


@pytest.mark.parametrize("scale", [1e30, 1e-30])
def test_extreme_gradient_magnitudes(scale, monkeypatch):
    """|dy| of the order of 1e30 / 1e-30: the power-of-two scale brings it into fp16's range -- no overflow to Inf, no flush to zero, still inside the rule"""
    x0, x1, a, d, y, dy = _direct_case("c20+12", scale)
    res = _direct_reference(x0, x1, a, d, y, dy, True)
    ours = ops.conv3d_bwd_weight_split(*_direct_args(x0, x1, a, d, y, dy, True))
    assert bool(torch.isfinite(ours).all()) and bool(ours.any())
    assert bool(((ours != 0).cpu() | (res[torch.float32] == 0)).all()), "a zero where the reference has a value"
    _check(f"split dy x {scale:g} direct d weight", res[torch.float64], res[torch.float32], ours, K_F16X2_BWD)
    real, stored, cout, dims, B = SCALE_LAYER
    conv, x0, x1, R = _layer_case(real, stored, cout, dims, B, r_scale=[scale, scale])
    _check_layer(f"dy x {scale:g} layer", conv, x0, x1, R, real, stored, monkeypatch)


def test_mixed_magnitudes_inside_one_sample():
    """|dy| from 1e-30 to 1e30 inside every sample (log-uniform): finite, and not all zeros where the reference is not; the elements far below the
    maximum are below one ulp of the result either way, so the rule holds as well"""
    x0, x1, a, d, y, dy = _direct_case("c20+12")
    mag = 10.0 ** (torch.rand(dy.shape, generator=_gen(5)) * 60 - 30)
    dy = dy * mag
    res = _direct_reference(x0, x1, a, d, y, dy, True)
    ours = ops.conv3d_bwd_weight_split(*_direct_args(x0, x1, a, d, y, dy, True))
    assert bool(torch.isfinite(ours).all()) and bool(ours.any())
    _check("split dy 1e-30 .. 1e30 direct d weight", res[torch.float64], res[torch.float32], ours, K_F16X2_BWD)


def test_a_nan_in_dy_is_never_quietly_finite():
    """one NaN in dy: every dW entry of its output channel is non-finite and no other; dX is non-finite in the 3 x 3 x 3 neighbourhood, exactly where the
    fp32 kernel's is; through the layer every gradient has the fp32 path's finite pattern"""
    x0, x1, a, d, y, dy = _direct_case("c20+12")
    B, cout = dy.shape[:2]
    b, co, z, yy, x = 1, 5, 2, 3, 4
    y[b, co, z, yy, x] = 1.0
    dy[b, co, z, yy, x] = float("nan")
    dw = ops.conv3d_bwd_weight_split(*_direct_args(x0, x1, a, d, y, dy, True))
    finite = torch.isfinite(dw).reshape(cout, -1)
    assert not bool(finite[co].any()), "dW[co] must be non-finite throughout"
    assert bool(finite[torch.arange(cout) != co].all())
    # the data gradient, called as the layer calls it
    w = torch.randn(cout, 32, 3, 3, 3, generator=_gen(9)).to(DEV)
    yd, dyd = _cl(y).to(DEV), _cl(dy).to(DEV)
    g, gmax, scale, inv = ops.relu_mask_max(yd, dyd)
    assert bool(torch.isfinite(gmax).all()) and bool(torch.isfinite(scale).all()), "the NaN must not decide the scale"
    dx = ops.conv3d_bwd_data_split(g, scale, inv, ops.pack_conv_weight_bwd_data_split(w), 32)
    ref = ops.conv3d_bwd_data(ops.relu_mask(yd, dyd), ops.pack_conv_weight_bwd_data(w), 32)
    bad = ~torch.isfinite(dx)
    assert torch.equal(bad, ~torch.isfinite(ref))
    want = torch.zeros_like(bad)
    want[b, z - 1:z + 2, yy - 1:yy + 2, x - 1:x + 2, :] = True
    assert torch.equal(bad, want)
    # through the layer
    real, stored, cout, dims, B = SCALE_LAYER
    conv, x0, x1, R = _layer_case(real, stored, cout, dims, B)
    y0, _ = _hip_layer(conv, x0, x1, R, stored, FP32)
    pos = (y0[1, :, :, :, 3] > 0).nonzero()[0]
    R[1, 3, pos[0], pos[1], pos[2]] = float("nan")
    _, gs = _hip_layer(conv, x0, x1, R, stored, SPLIT)
    _, gf = _hip_layer(conv, x0, x1, R, stored, FP32)
    for s, f in zip(gs, gf):
        assert torch.equal(torch.isfinite(s), torch.isfinite(f))
    assert not bool(torch.isfinite(gs[2][3]).any())


# ------------------------------------------------------------------------------------------------ 4. compositions with shared selections
@pytest.mark.parametrize("which", ["main", "padded_4x12x10", "main_4x8x12"])
def test_composition_shared_selections_split(which, monkeypatch):
    model, x, R = _composition_inputs(which, 0, B=COMPOSITIONS[which].get("B", 2))
    mg = copy.deepcopy(model).to(DEV)
    sel = hip_selections(mg, x, FP32)
    g64, o64 = restated_unet_grads(model, x, R, torch.float64, selections=sel)
    g32, _ = restated_unet_grads(model, x, R, torch.float32, selections=sel)
    spy = _Spy(monkeypatch)
    gh, oh = hip_unet_grads(mg, x, R, SPLIT)
    layers = 2 * (len(model.encoders) + len(model.decoders))
    assert spy.calls == {"conv3d_bwd_weight_split": layers, "conv3d_bwd_data_split": layers, "conv3d_bwd_weight": 0, "conv3d_bwd_data": 0}, spy.calls
    assert float((oh.double().cpu() - o64).abs().max()) <= 1e-4 * float(o64.abs().max())
    ratios = _compare_all(f"split unet {which} shared", g64, g32, gh, K_F16X2_BWD)
    print(f"[grad-error] split unet {which} shared: largest ratio to e32 {max(ratios.values()):.2f}")
    gh2, _ = hip_unet_grads(mg, x, R, SPLIT)
    for k in gh:
        assert torch.equal(gh[k], gh2[k]), k


# ------------------------------------------------------------------------------------------------ 5. nothing else moved
def test_fp32_mode_is_todays_backward_and_the_forward_never_moves(monkeypatch):
    model, x, R = _composition_inputs("padded", 0)
    mg = copy.deepcopy(model).to(DEV)
    spy = _Spy(monkeypatch)
    ga, oa = hip_unet_grads(mg, x, R, AR.Arith())
    gb, ob = hip_unet_grads(mg, x, R, AR.Arith(conv_grad_mode="fp32"))
    assert spy.calls["conv3d_bwd_weight_split"] == 0 and spy.calls["conv3d_bwd_data_split"] == 0 and spy.calls["conv3d_bwd_weight"] > 0
    assert torch.equal(oa, ob)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    gs, os_ = hip_unet_grads(mg, x, R, AR.Arith(conv_grad_mode="f16x2"))
    assert torch.equal(os_, oa), "the flag touches the backward only"
    assert spy.calls["conv3d_bwd_weight_split"] > 0 and spy.calls["conv3d_bwd_data_split"] > 0
    assert any(not torch.equal(gs[k], ga[k]) for k in ga)
    with torch.no_grad():
        assert torch.equal(A.unet3d(mg, x.to(DEV), arith=AR.Arith(conv_grad_mode="f16x2")), A.unet3d(mg, x.to(DEV), arith=AR.Arith()))


def test_split_backward_with_device_packs_does_not_synchronise():
    """after an in-place weight update, forward and backward of a two-source layer under device_packs + conv_grad_mode = "f16x2": the maxima, the scales
    and the data gradient's pack are all found / built on the device -- torch's synchronisation check stays silent"""
    real, stored, cout, dims, B = SCALE_LAYER
    conv, x0, x1, R = _layer_case(real, stored, cout, dims, B)
    cg = copy.deepcopy(conv).to(DEV)
    arith = AR.Arith(device_packs=True, conv_grad_mode="f16x2")
    s0, s1 = _to_stored_cl(x0, stored[0]).to(DEV).requires_grad_(True), _to_stored_cl(x1, stored[1]).to(DEV).requires_grad_(True)
    Rd = _to_stored_cl(R, stored_channels(cout)).to(DEV)
    leaves = [s0, s1, cg.conv.weight, cg.groupnorm.weight, cg.groupnorm.bias]
    warm = torch.autograd.grad(A.conv3d_gcr(cg, s0, s1, arith=arith), leaves, Rd)          # everything that is built once exists
    with torch.no_grad():
        cg.conv.weight.mul_(1.01)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        got = torch.autograd.grad(A.conv3d_gcr(cg, s0, s1, arith=arith), leaves, Rd)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert all(bool(torch.isfinite(t).all()) for t in got) and not torch.equal(got[0], warm[0])


# ------------------------------------------------------------------------------------------------ 6. a training step
def test_train_step_with_the_split_backward(monkeypatch):
    """train_pipeline.train_step of the smallest model under conv_grad_mode = "f16x2": every trainable tensor's gradient against
    tests/pipeline_train_reference.py's restatement (the parameters and BatchNorm buffers the step started from, the step's own ReLU masks), finite loss"""
    import math

    import pipeline_train_reference as PR
    from garmentnets_amd import train_pipeline as TP
    from test_gpu_train_pipeline import FIRST, _first_stage_relus, _setup
    cpu_model, batch_cpu = _setup("A")
    model = copy.deepcopy(cpu_model).to(DEV).requires_grad_(True).train()
    model.arith = model.arith.replace(conv_grad_mode="f16x2")
    batch = batch_cpu.to(DEV)
    buffers = {k: v.detach().cpu().clone() for k, v in model.named_buffers()}
    start = {k: v.detach().cpu().clone() for k, v in model.named_parameters()}
    skip, p2 = _first_stage_relus(model, batch)
    nd, agg = p2["nocs_data"], model.volume_agg
    rows, flat = ops.grid_features(nd.x, nd.pos.contiguous(), nd.sim_points.float().contiguous(), nd.pred_confidence.contiguous(), nd.batch,
                                   agg.lower_corner, agg.upper_corner, agg.grid_shape, True, True)
    rows, flat = rows.cpu().contiguous(), flat.cpu()
    model.train()
    spy = _Spy(monkeypatch)
    with PR.record_second_stage() as rec:
        metrics = TP.train_step(model, model.configure_optimizers(), batch)
    assert math.isfinite(metrics["loss"])
    assert spy.calls["conv3d_bwd_weight_split"] == 6 and spy.calls["conv3d_bwd_data_split"] == 6 and spy.calls["conv3d_bwd_weight"] == 0
    masks = ([(r > 0).cpu() for r in rec["r"][skip:]], rec["conv"])

    def restated(dtype):
        P = {k: v.to(dtype).requires_grad_(True) for k, v in start.items() if not k.startswith(FIRST)}
        ls = PR.Restated(cpu_model, P, buffers, dtype, True, masks).loss(rows, flat, batch_cpu)
        return float(ls.detach()), dict(zip(P, torch.autograd.grad(ls, list(P.values()))))
    l64, g64 = restated(torch.float64)
    _, g32 = restated(torch.float32)
    assert abs(metrics["loss"] - l64) <= 1e-5 * abs(l64)
    failed, ratios = [], []
    for name, p in model.named_parameters():
        if name.startswith(FIRST):
            continue
        assert p.grad is not None, name
        try:
            ratios.append(_check(f"split train step {name}", g64[name], g32[name], p.grad, K_F16X2_BWD))
        except AssertionError as e:
            failed.append(str(e.args[0])[:200])
    assert len(ratios) + len(failed) == len(g64)
    if ratios:
        print(f"[grad-error] split train step: {len(g64)} tensors, ours / torch-fp32 {min(ratios):.2f} - {max(ratios):.2f}")
    assert not failed, failed
