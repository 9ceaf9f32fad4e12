"""GPU (-m gpu): gradients of the 3-D UNet (csrc/unet_grad.hip, autograd.conv3d_gcr / max_pool3d_2 / unet3d).

Reference: a plain-torch restatement built here from nn.functional (group_norm, conv3d, relu, max_pool3d, interpolate(mode='nearest'), cat) on the
model's own parameters, run on the CPU in fp64 and in fp32.  Error rule (tests/test_gpu_autograd.py::_check_weighted): ours against fp64 at most
4 x (torch-fp32 against fp64) + 1 fp32 ulp of the largest gradient, printed as `[grad-error] ...` before it is asserted.  No element is excluded.

Layer level: the restatement is handed the ReLU mask of the HIP forward (y_hip > 0), so both sides differentiate the same piecewise-linear map.
Composition: each side forms its own masks and pool winners; a flipped ReLU / pool winner near a tie is a real difference, carried by the torch-fp32
run as well.  Stability of that measure: the fp32-against-fp64 restatement alone on the CPU of the build machine (print_cpu_e32: e32 of d x, and the
largest e32 / max |g| over all tensors), per seed of _composition_inputs:
    f_maps (16, 48), 8^3, B = 2:        seeds 0 / 1 / 2: e32(d x) 2.153e-06 / 2.011e-06 / 1.987e-06 (relative 1.8e-06 / 1.6e-06 / 1.6e-06): stable.
    f_maps (32, 64, 128), 16^3, B = 2:  seeds 0 / 1 / 2: e32(d x) 1.585e-02 / 4.188e-06 / 2.123e-02 -- NOT stable: the measure is bimodal.  Over seeds
        0..11 it is either 4e-06 (seeds 1, 5, 8, 9, 10: the fp32 run flips no ReLU / pool winner) or 0.6-5e-02 (seeds 0, 2, 3, 4, 6, 7, 11: it flips at
        least one).  A seed of the first kind would hold OUR run to 4 x 4e-06 although a different fp32 rounding order may flip a winner the torch run
        did not; so the inputs are taken from the second kind, where the measure is stable: seeds 0 / 2 / 4: e32(d x) 1.585e-02 / 2.123e-02 / 1.714e-02
        (relative 1.0e-02 / 1.3e-02 / 9.1e-03).  The test runs seed 0.  The sharp check of the arithmetic is the layer level above, where no flip exists.
Default arithmetic (f16x2 forward, fp32 backward), measured on an MI355X: largest (ours - fp64) / e32 over all tensors 1.15 (main) and 1.60 (padded);
asserted with k = 2, the measured ratio rounded up to the next power of two (strict-fp32 forward: 1.15 and 1.88 under the rule's 4).
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from garmentnets_amd import arith as AR, autograd as A  # noqa: E402
from garmentnets_amd.components.unet3d import Abstract3DUNet, SingleConv, stored_channels  # noqa: E402

DEV = "cuda:0"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _check(name, ref64, t32, ours, factor=4):
    """ours against fp64 <= factor x (torch-fp32 against fp64) + 1 fp32 ulp of the largest gradient; prints before it asserts; returns the ratio"""
    ref64, t32, ours = ref64.double().cpu(), t32.double().cpu(), ours.double().cpu()
    assert ref64.shape == ours.shape, (name, ref64.shape, ours.shape)
    assert bool(torch.isfinite(ours).all()), name
    e32 = float((t32 - ref64).abs().max())
    eo = float((ours - ref64).abs().max())
    ulp = float(np.spacing(np.float32(ref64.abs().max())))
    bound = "none (printed only)" if factor is None else f"{factor * e32 + ulp:.3e}"
    print(f"[grad-error] {name}: torch-fp32 {e32:.3e}  hip {eo:.3e}  ulp(max |g|) {ulp:.3e}  bound {bound}  ratio {eo / max(e32, 1e-300):.2f}")
    if factor is not None:
        assert eo <= factor * e32 + ulp, (name, eo, e32, ulp)
    return eo / max(e32, 1e-300)


# ------------------------------------------------------------------------------------------------ restatement (plain torch, any dtype, CPU, NCDHW)
def r_layer(x0, x1, w, gamma, beta, groups, eps, mask=None):
    x = x0 if x1 is None else torch.cat((x0, F.interpolate(x1, scale_factor=2, mode="nearest")), 1)
    h = F.conv3d(F.group_norm(x, groups, gamma, beta, eps), w, padding=1)
    return F.relu(h) if mask is None else h * mask


def r_unet(model, P, x, selections=None):
    """selections: (ReLU masks per layer in execution order, pool winner indices per level) taken from the HIP forward (hip_selections): the restatement
    then differentiates the same piecewise-linear map as the HIP run, whatever the dtype; None: it forms its own"""
    masks, winners = (None, None) if selections is None else (iter(selections[0]), iter(selections[1]))

    def double_conv(prefix, dc, x0, x1=None):
        for k, sc in (("SingleConv1", dc.SingleConv1), ("SingleConv2", dc.SingleConv2)):
            n = f"{prefix}.basic_module.{k}"
            x0 = r_layer(x0, x1, P[n + ".conv.weight"], P[n + ".groupnorm.weight"], P[n + ".groupnorm.bias"], sc.groupnorm.num_groups, sc.groupnorm.eps,
                         mask=None if masks is None else next(masks).to(x0.dtype))
            x1 = None
        return x0
    feats = []
    for i, enc in enumerate(model.encoders):
        if i > 0 and winners is not None:
            idx = next(winners)
            x = x.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
        elif i > 0:
            x = F.max_pool3d(x, 2)
        x = double_conv(f"encoders.{i}", enc.basic_module, x)
        feats.insert(0, x)
    for i, dec in enumerate(model.decoders):
        x = double_conv(f"decoders.{i}", dec.basic_module, feats[i + 1], x)
    return F.conv3d(x, P["final_conv.weight"], P["final_conv.bias"])


def _randomise_norms(module, g):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))


def _model(in_ch, out_ch, f_maps, seed, **kw):
    torch.manual_seed(seed)
    model = Abstract3DUNet(in_ch, out_ch, f_maps=f_maps, num_groups=8, **kw)
    _randomise_norms(model, _gen(seed + 1000))
    return model


def hip_selections(model_gpu, x, arith):
    """the ReLU masks (y > 0 on the real channels, NCDHW, CPU) of every layer and ATen's max-pool winners over the HIP activations, from the layers
    autograd.unet3d runs (its own _conv / _pool, under no_grad: the same launches, the same bits)"""
    masks, winners, feats = [], [], []

    def conv(sc, *args):
        v, st = A._conv(sc, *args, arith)
        masks.append((v[..., :sc.conv.out_channels] > 0).permute(0, 4, 1, 2, 3).cpu())
        return v, st
    with torch.no_grad():
        v = x.to(DEV).permute(0, 2, 3, 4, 1).contiguous()
        if v.shape[-1] % 16 != 0:
            v = F.pad(v, (0, stored_channels(v.shape[-1]) - v.shape[-1]))
        stats, real = None, None
        for enc in model_gpu.encoders:
            dc = enc.basic_module
            if enc.pooling is not None:
                winners.append(F.max_pool3d(v[..., :real].permute(0, 4, 1, 2, 3).cpu(), 2, return_indices=True)[1])
                v, stats = A._pool(v)
            v, stats = conv(dc.SingleConv1, v, None, stats, None)
            v, stats = conv(dc.SingleConv2, v, None, stats, None)
            real = dc.SingleConv2.conv.out_channels
            feats.insert(0, (v, stats))
        for dec, (skip, ss) in zip(model_gpu.decoders, feats[1:]):
            dc = dec.basic_module
            v, stats = conv(dc.SingleConv1, skip, v, ss, stats)
            v, stats = conv(dc.SingleConv2, v, None, stats, None)
    return masks, winners


def restated_unet_grads(model, x, R, dtype, fn=None, selections=None):
    """{name: gradient} of sum(r_unet(x) * R) (or of fn(r_unet's output)) for 'x' and every parameter, on the CPU in dtype"""
    P = {n: p.detach().cpu().to(dtype).requires_grad_(True) for n, p in model.named_parameters()}
    xx = x.detach().cpu().to(dtype).requires_grad_(True)
    out = r_unet(model, P, xx, selections)
    loss = (out * R.to(dtype)).sum() if fn is None else fn(out)
    names = ["x"] + list(P)
    return dict(zip(names, torch.autograd.grad(loss, [xx] + list(P.values())))), out.detach()


def hip_unet_grads(model_gpu, x, R, arith, fn=None):
    xx = x.detach().to(DEV).requires_grad_(True)
    out = A.unet3d(model_gpu, xx, arith=arith)
    assert out.grad_fn is not None
    loss = (out * R.to(DEV)).sum() if fn is None else fn(out)
    names = ["x"] + [n for n, _ in model_gpu.named_parameters()]
    return dict(zip(names, torch.autograd.grad(loss, [xx] + [p for _, p in model_gpu.named_parameters()]))), out.detach()


COMPOSITIONS = {"main": dict(in_ch=32, out_ch=8, f_maps=(32, 64, 128), n=16), "padded": dict(in_ch=8, out_ch=5, f_maps=(16, 48), n=8),
                # stored widths 64 / 96 / 160 / 256: the max-pool without a statistics epilogue (96), gn_channel_stats_any, a 256-channel virtual concat
                "wide": dict(in_ch=16, out_ch=4, f_maps=(96, 160), n=8)}


def _composition_inputs(which, seed):
    """the model and inputs of a composition case; B = 2.  tests/ holds no CPU-only runner: print_cpu_e32() (no GPU needed) prints the three-seed stability figures of the module docstring"""
    c = COMPOSITIONS[which]
    model = _model(c["in_ch"], c["out_ch"], c["f_maps"], seed)
    g = _gen(seed + 7)
    x = torch.randn(2, c["in_ch"], c["n"], c["n"], c["n"], generator=g)
    R = torch.randn(2, c["out_ch"], c["n"], c["n"], c["n"], generator=g)
    return model, x, R


def print_cpu_e32():
    for which in ("main", "padded"):
        for seed in (0, 1, 2):
            model, x, R = _composition_inputs(which, seed)
            g64, _ = restated_unet_grads(model, x, R, torch.float64)
            g32, _ = restated_unet_grads(model, x, R, torch.float32)
            rel = max(float((g32[k].double() - g64[k]).abs().max()) / float(g64[k].abs().max()) for k in g64)
            ex = float((g32["x"].double() - g64["x"]).abs().max())
            print(f"[cpu-e32] {which} seed {seed}: max over tensors of e32 / max|g| = {rel:.3e}   e32(d x) = {ex:.3e}")


# ------------------------------------------------------------------------------------------------ 1. one layer, linear parts isolated
def _to_stored_cl(x, stored):
    """(B, C, D, H, W) -> channel-last [B][D][H][W][stored], zeros on the pads"""
    v = x.permute(0, 2, 3, 4, 1).contiguous()
    return F.pad(v, (0, stored - v.shape[-1])) if stored != v.shape[-1] else v


@pytest.mark.parametrize("real,stored,cout,dims", [
    ((32,), (32,), 64, (8, 16, 16)),           # one source
    ((32, 64), (32, 64), 64, (8, 8, 8)),       # two sources, 8 groups of 12 channels: group 2 (channels 24..35) straddles src0 / src1
    ((16,), (16,), 48, (8, 8, 8)),             # padded output width (stored 64), a 16-wide input: the transposed pack padded to 32 columns
    ((48,), (64,), 32, (4, 8, 8)),             # padded input
    ((48, 16), (64, 32), 48, (8, 8, 8)),       # both sources and the output padded, the groups (8 per group) over the real channels
])
def test_layer_gradients(real, stored, cout, dims):
    g = _gen(sum(real) + cout)
    B = 2
    conv = SingleConv(sum(real), cout)
    conv.in_real = real
    _randomise_norms(conv, g)
    x0 = torch.randn(B, real[0], *dims, generator=g) * 1.5 + 0.3
    x1 = torch.randn(B, real[1], *(n // 2 for n in dims), generator=g) if len(real) > 1 else None
    cs = stored_channels(cout)
    R = torch.randn(B, cout, *dims, generator=g)
    cg = copy.deepcopy(conv).to(DEV)
    s0 = _to_stored_cl(x0, stored[0]).to(DEV).requires_grad_(True)
    s1 = None if x1 is None else _to_stored_cl(x1, stored[1]).to(DEV).requires_grad_(True)
    y = A.conv3d_gcr(cg, s0, s1, arith=AR.DEFAULT.strict_fp32())
    assert tuple(y.shape) == (B, *dims, cs) and y.grad_fn is not None
    assert not bool(y[..., cout:].any())
    leaves = [s0] + ([s1] if s1 is not None else []) + [cg.conv.weight, cg.groupnorm.weight, cg.groupnorm.bias]
    gh = list(torch.autograd.grad((y * _to_stored_cl(R, cs).to(DEV)).sum(), leaves))
    mask = (y[..., :cout] > 0).permute(0, 4, 1, 2, 3).cpu()
    res = {}
    for dtype in (torch.float64, torch.float32):
        lv = [t.detach().to(dtype).requires_grad_(True) for t in [x0] + ([x1] if x1 is not None else []) + [conv.conv.weight, conv.groupnorm.weight, conv.groupnorm.bias]]
        a0, a1 = lv[0], (lv[1] if x1 is not None else None)
        out = r_layer(a0, a1, lv[-3], lv[-2], lv[-1], conv.groupnorm.num_groups, conv.groupnorm.eps, mask=mask.to(dtype))
        res[dtype] = (out.detach(), torch.autograd.grad((out * R.to(dtype)).sum(), lv))
    # the restatement's forward against the HIP forward (a wrong restatement cannot pass quietly)
    yr = res[torch.float64][0].permute(0, 2, 3, 4, 1)
    assert float((y[..., :cout].double().cpu() - yr).abs().max()) <= 1e-4 * float(yr.abs().max())
    names = ["d src0"] + (["d src1"] if x1 is not None else []) + ["d weight", "d gamma", "d beta"]
    for i, name in enumerate(names):
        ours = gh[i]
        if name.startswith("d src"):
            r = real[int(name[-1])]
            assert not bool(ours[..., r:].any()), f"{name}: pad gradients must be exact zeros"
            ours = ours[..., :r].permute(0, 4, 1, 2, 3)
        _check(f"layer {real}->{cout} {name}", res[torch.float64][1][i], res[torch.float32][1][i], ours)


# ------------------------------------------------------------------------------------------------ 2. max-pool: exact
def test_max_pool_gradient_is_bit_exact_with_ties_and_a_nan():
    g = _gen(5)
    x = torch.randn(2, 32, 8, 8, 8, generator=g)
    x[:, :8, 0:2, 0:2, 0:2] = 1.25                 # whole windows tied: the first voxel in (z, y, x) order wins
    x[:, 8:16, :, :, 1::2] = x[:, 8:16, :, :, 0::2].clone()  # pairs tied along x
    x[0, :, 2:4, 2:4, 2:4] = x[0, :, 2:3, 2:3, 2:3].clone()
    x[1, 3, 5, 4, 6] = float("nan")                # a NaN wins its window
    x[1, 4, 4, 4, 4] = float("nan")
    x[1, 4, 5, 5, 5] = float("nan")                # two NaNs in one window: ATen keeps the later one
    go = torch.randn(2, 32, 4, 4, 4, generator=g)
    xr = x.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(F.max_pool3d(xr, 2), xr, go)
    xs = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV).requires_grad_(True)
    out = A.max_pool3d_2(xs)
    (ours,) = torch.autograd.grad(out, xs, go.permute(0, 2, 3, 4, 1).contiguous().to(DEV))
    assert torch.equal(ours.cpu().permute(0, 4, 1, 2, 3), ref)


# ------------------------------------------------------------------------------------------------ 3. composition
def _compare_all(tag, g64, g32, gh, factor=4):
    assert set(gh) == set(g64)
    return {k: _check(f"{tag} {k}", g64[k], g32[k], gh[k], factor) for k in g64}


@pytest.mark.parametrize("which", ["main", "padded"])
def test_composition_strict_fp32(which):
    model, x, R = _composition_inputs(which, 0)
    g64, o64 = restated_unet_grads(model, x, R, torch.float64)
    g32, _ = restated_unet_grads(model, x, R, torch.float32)
    mg = copy.deepcopy(model).to(DEV)
    gh, oh = hip_unet_grads(mg, x, R, AR.DEFAULT.strict_fp32())
    assert float((oh.double().cpu() - o64).abs().max()) <= 1e-4 * float(o64.abs().max())
    _compare_all(f"unet {which} fp32", g64, g32, gh)
    # determinism: identical calls, identical bits, every tensor
    gh2, _ = hip_unet_grads(mg, x, R, AR.DEFAULT.strict_fp32())
    for k in gh:
        assert torch.equal(gh[k], gh2[k]), k


@pytest.mark.parametrize("which,seed", [("main", 0), ("main", 1), ("padded", 0), ("wide", 0)])
def test_composition_shared_selections(which, seed):
    """The sharp check through the depth of the net: the restatement is handed the HIP forward's ReLU masks and pool winners, so both sides differentiate
    the same piecewise-linear map, no winner can flip on either side, and e32 is the plain fp32 rounding error (about 1e-06 of the largest gradient)
    for every seed -- the rule's 4 x e32 + ulp then holds every tensor of the 3-level net to that.  Strict-fp32 forward."""
    model, x, R = _composition_inputs(which, seed)
    mg = copy.deepcopy(model).to(DEV)
    fp32 = AR.DEFAULT.strict_fp32()
    sel = hip_selections(mg, x, fp32)
    g64, o64 = restated_unet_grads(model, x, R, torch.float64, selections=sel)
    g32, _ = restated_unet_grads(model, x, R, torch.float32, selections=sel)
    gh, oh = hip_unet_grads(mg, x, R, fp32)
    assert float((oh.double().cpu() - o64).abs().max()) <= 1e-4 * float(o64.abs().max())
    rel = max(float((g32[k].double() - g64[k]).abs().max()) / float(g64[k].abs().max()) for k in g64)
    print(f"[grad-error] unet {which} seed {seed} shared selections: largest e32 / max |g| over the tensors {rel:.3e}")
    _compare_all(f"unet {which} seed {seed} shared", g64, g32, gh)


@pytest.mark.parametrize("half", [False, True])
def test_groupnorm_bwd_apply_accumulates(half):
    """out= given: the result is added to what it holds, one fp32 add per element"""
    from garmentnets_amd import ops
    g = _gen(31 + half)
    B, D, C, ld, goff, coff = 2, 4, 32, 96, 32, 64
    k = 2 if half else 1
    dxn = torch.randn(B, k * D, k * D, k * D, ld, generator=g).to(DEV)
    x = torch.randn(B, D, D, D, C, generator=g).to(DEV)
    p, q, r = (torch.randn(B, 128, generator=g).to(DEV) for _ in range(3))
    held = torch.randn(B, D, D, D, C, generator=g).to(DEV)
    plain = ops.groupnorm_bwd_apply(dxn, goff, x, p, q, r, coff, half=half)
    out = held.clone()
    assert ops.groupnorm_bwd_apply(dxn, goff, x, p, q, r, coff, half=half, out=out) is out
    assert torch.equal(out, held + plain)
    fine = dxn[..., goff:goff + C].double()
    if half:
        fine = fine.view(B, D, 2, D, 2, D, 2, C).sum((2, 4, 6))
    ref = fine * p[:, None, None, None, coff:coff + C].double() + k ** 3 * (x.double() * q[:, None, None, None, coff:coff + C].double()
                                                                          + r[:, None, None, None, coff:coff + C].double())
    assert float((plain.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


K_F16X2 = 2         # the asserted factor of the default-arithmetic test: the measured ratio (1.15 / 1.60) rounded up to the next power of two


@pytest.mark.parametrize("which", ["main", "padded"])
def test_composition_default_arithmetic(which):
    """f16x2 forward, fp32 backward.  Measured largest (ours - fp64) / e32 over all tensors: 1.15 (main), 1.60 (padded) -> k = 2 (module docstring)."""
    model, x, R = _composition_inputs(which, 0)
    g64, _ = restated_unet_grads(model, x, R, torch.float64)
    g32, _ = restated_unet_grads(model, x, R, torch.float32)
    mg = copy.deepcopy(model).to(DEV)
    gh, oh = hip_unet_grads(mg, x, R, None)
    with torch.no_grad():
        assert torch.equal(oh, mg(x.to(DEV))), "the differentiable forward must be model.forward's bits"
    ratios = _compare_all(f"unet {which} f16x2", g64, g32, gh, K_F16X2)
    print(f"[grad-error] unet {which} f16x2: largest ratio to e32 {max(ratios.values()):.2f}")
    gh2, _ = hip_unet_grads(mg, x, R, None)
    for k in gh:
        assert torch.equal(gh[k], gh2[k]), k


@pytest.mark.parametrize("which", ["padded", "wide"])
def test_no_grad_path_is_model_forward_and_saves_nothing(which):
    model, x, _ = _composition_inputs(which, 3)
    mg = copy.deepcopy(model).to(DEV)
    xd = x.to(DEV)
    with torch.no_grad():
        ref = mg(xd)
        out = A.unet3d(mg, xd)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, ref)
    out = A.unet3d(mg, xd.clone().requires_grad_(True))
    assert out.grad_fn is not None and torch.equal(out.detach(), ref)
    # an input that carries its channel-padded storage and the producer's statistics, as the volume aggregator's does: honoured on the grad path too
    from garmentnets_amd import ops
    from garmentnets_amd.components.unet3d import to_stored
    carried = xd.clone()
    carried._gn_stored = to_stored(xd.permute(0, 2, 3, 4, 1).contiguous(), (xd.shape[1],), (stored_channels(xd.shape[1]),)).contiguous()
    carried._gn_stats = ops.channel_stats(carried._gn_stored)
    with torch.no_grad():
        ref_c = mg(carried)
    out = A.unet3d(mg, carried)
    assert out.grad_fn is not None and torch.equal(out.detach(), ref_c)
    mg.requires_grad_(False)
    out = A.unet3d(mg, xd)                          # grad mode on, nothing requires a gradient
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, ref)


# ------------------------------------------------------------------------------------------------ 4. the end of the chain
def test_second_stage_chain_gradient():
    """autograd.scatter (mean) -> autograd.unet3d -> autograd.grid_sample_points -> MSE: gradient to the scattered rows"""
    def r_scatter_mean(src, cell, cells):
        mask = (cell[None, :] == torch.arange(cells)[:, None]).to(src.dtype)
        return (mask @ src) / mask.sum(1).clamp(min=1)[:, None]

    def r_sample(volume, query):
        nb, m = query.shape[:2]
        s = F.grid_sample(volume, (2.0 * query - 1.0).view(nb, m, 1, 1, 3), mode="bilinear", padding_mode="border", align_corners=True)
        return s.view(nb, volume.shape[1], m).permute(0, 2, 1)
    g = _gen(61)
    B, n, C, G, M, CO = 2, 600, 32, 16, 300, 8
    model = _model(C, CO, (32, 64), 11)
    feat = torch.randn(B * n, C, generator=g)
    cell = torch.randint(0, G, (B * n, 3), generator=g)
    cell[:200] = cell[0]
    batch = torch.arange(B).repeat_interleave(n)
    flat = ((batch * G + cell[:, 0]) * G + cell[:, 1]) * G + cell[:, 2]
    q = torch.rand(B, M, 3, generator=g) * 1.2 - 0.1
    tgt = torch.randn(B, M, CO, generator=g)
    res = {}
    for dtype in (torch.float64, torch.float32):
        P = {k: p.detach().to(dtype) for k, p in model.named_parameters()}
        f = feat.to(dtype).requires_grad_(True)
        vol = r_scatter_mean(f, flat, B * G ** 3).view(B, G, G, G, C).permute(0, 4, 1, 2, 3)
        loss = F.mse_loss(r_sample(r_unet(model, P, vol), q.to(dtype)), tgt.to(dtype))
        res[dtype] = (float(loss), torch.autograd.grad(loss, f)[0])
    mg = copy.deepcopy(model).to(DEV)

    def hip():
        f = feat.to(DEV).requires_grad_(True)
        vol = A.scatter(f.t(), flat.to(DEV), -1, B * G ** 3, "mean").view(C, B, G, G, G).permute(1, 0, 2, 3, 4)
        out = A.unet3d(mg, vol, arith=AR.DEFAULT.strict_fp32())
        loss = F.mse_loss(A.grid_sample_points(out, q.to(DEV)), tgt.to(DEV))
        return float(loss), torch.autograd.grad(loss, f)[0]
    lh, gh = hip()
    assert abs(lh - res[torch.float64][0]) <= 1e-5 * abs(res[torch.float64][0])
    _check("second stage chain d rows", res[torch.float64][1], res[torch.float32][1], gh)
    assert torch.equal(gh, hip()[1])


# ------------------------------------------------------------------------------------------------ 5. the reference's training shape, once
def test_reference_training_shape():
    """the reference's second-stage UNet (unet3d_params: 128 in, 128 out, f_maps = 32, 4 levels) at 32^3, B = 2: runs, finite, d conv.weight of the
    first and the last layer and the final convolution's d weight (128 x 32) / d bias against fp64"""
    model = _model(128, 128, 32, 21, num_levels=4)
    g = _gen(22)
    x = torch.randn(2, 128, 32, 32, 32, generator=g)
    R = torch.randn(2, 128, 32, 32, 32, generator=g)
    g64, _ = restated_unet_grads(model, x, R, torch.float64)
    g32, _ = restated_unet_grads(model, x, R, torch.float32)
    gh, _ = hip_unet_grads(copy.deepcopy(model).to(DEV), x, R, AR.DEFAULT.strict_fp32())
    for k, v in gh.items():
        assert bool(torch.isfinite(v).all()), k
    last = f"decoders.{len(model.decoders) - 1}.basic_module.SingleConv2.conv.weight"
    for k in ("encoders.0.basic_module.SingleConv1.conv.weight", last, "final_conv.weight", "final_conv.bias"):
        _check(f"training shape {k}", g64[k], g32[k], gh[k])
