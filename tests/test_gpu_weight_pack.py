"""GPU (-m gpu): the static split-operand weight packs built on the device (csrc/weight_pack.hip, ops.pack_*_device, arith.Arith.device_packs).

1. Bit equality with the host builders (ops.pack_conv_weight_split, pack_conv_weight_split_wino, polyphase_weights + pack_upconv_weight): torch.equal on
   the int16 patterns (zero steps included) and on out_scale.  The inputs are conditioned ON THE CPU, and the conditions asserted there before anything
   is compared: (i) every row maximum the host takes a log2 of has floor(log2(m)) == frexp exponent - 1 (the host's log2 rounds up a few ulps below a
   power of two: the one documented difference, test 2); (ii) the non-zero magnitudes inside every 3-term (Winograd) and 8-term (polyphase) sum spread
   over at most 2^24, so the fp64 sums are exact and order-free (24 + 24 + 3 < 53).  No NaN: its payload is not part of the contract.
2. The documented scale rule where the host differs: rows whose maximum is nextafter(2^-4, 0) / nextafter(2^-10, 0).  No comparison with the host.
3. SingleConv takes the device packs on every plan that reads a static pack, asserted inside the test; bit-identical output, also after an in-place
   update of the weight.
4. A UNet forward after a weight update issues no synchronising call with device_packs (torch.cuda.set_sync_debug_mode("error")) -- and does with the
   host builders, which shows the detector works.
5. Three training steps of the small pipeline model (the shapes of tests/test_gpu_train_pipeline.py) give the same losses and parameters bit for bit.
"""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import ops, synthetic, train_pipeline as TP  # noqa: E402
from garmentnets_amd.arith import SPLIT_BF16X2, SPLIT_BF16X3, SPLIT_F16X2, Arith  # noqa: E402
from garmentnets_amd.batch import Batch  # noqa: E402
from garmentnets_amd.components import unet3d as U  # noqa: E402
from garmentnets_amd.networks.conv_implicit_wnf import ConvImplicitWNFPipeline  # noqa: E402

DEV = "cuda:0"
MODES = {"f16x2": SPLIT_F16X2, "bf16x2": SPLIT_BF16X2, "bf16x3": SPLIT_BF16X3}
# (Cout, Cin): one slice and block; several slices and blocks; a real layer
PLAIN = {"one": (32, 16), "several": (96, 48), "layer": (128, 128)}
# (Cout, c0, c1)
POLY = {"small": (32, 32, 16), "larger": (64, 64, 128)}
# channel ranges [c_lo, c_lo + c_n) of the plain shapes (the second starts inside the weight) -- the polyphase shapes add [0, c0)
RANGES = {"several_head": ("several", 0, 32), "several_inner": ("several", 16, 32), "layer_head": ("layer", 0, 64)}
SETS = ("randn", "heavy_tail", "zero_row", "pow2_row", "tiny_elements")
ZERO_ROW, POW2_ROW = 3, 5


# ------------------------------------------------------------------------------------------------ inputs and their conditions (CPU)
def _floored(w):
    """non-zero magnitudes below 2^-20 of their row's maximum raised to it (exact: a power of two times the maximum)"""
    m = w.reshape(w.shape[0], -1).abs().amax(dim=1).view(-1, 1, 1, 1, 1) * 2.0 ** -20
    return torch.where((w != 0) & (w.abs() < m), torch.copysign(m.expand_as(w), w), w)


@functools.lru_cache(maxsize=None)
def weights(cout, cin, kind, c0=None):
    """the fp32 CPU weight (Cout, Cin, 3,3,3) of one input set; c0: the split point of a polyphase layer"""
    g = torch.Generator().manual_seed(cout * 1000 + cin + 17 * SETS.index(kind))
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.05
    if kind == "heavy_tail":
        # rows scaled by 2^0 .. 2^-12; inside a row magnitudes in [2^-19, 1.5): a spread below 2^20
        mag = (0.5 + torch.rand(w.shape, generator=g)) * torch.exp2(-torch.randint(0, 19, w.shape, generator=g).float())
        w = torch.copysign(mag, w) * 0.05 * torch.exp2(-(torch.arange(cout) % 13).float()).view(-1, 1, 1, 1, 1)
    if kind == "zero_row":
        w[ZERO_ROW] = 0
    if kind == "pow2_row":
        # the row maximum exactly 2^-3: of the plain row (and of its Winograd transform: position 0 is g0 itself) at tap (1, 1, 0) of channel 2, of
        # the merged row of parity class 0 (its coarse tap 0 is the fine tap (0, 0, 0) alone) at channel c0 + 1
        w[POW2_ROW] *= 0.1
        w[POW2_ROW, 2, 1, 1, 0] = 2.0 ** -3
        if c0 is not None:
            w[POW2_ROW, c0 + 1, 0, 0, 0] = 2.0 ** -3
    if kind == "tiny_elements":
        m = w.reshape(cout, -1).abs().amax(dim=1).view(-1, 1, 1, 1, 1) * 2.0 ** -20
        w[:, 1::5, :, :, 1] = m.expand_as(w)[:, 1::5, :, :, 1]
    w = _floored(w).contiguous()
    assert torch.isfinite(w).all()
    return w


def _assert_exponent_rule(m):
    """(i): where the host builder takes floor(log2(m)) of a row maximum, it is the exponent field's value"""
    m = m.reshape(-1)
    m = m[m > 0]
    assert torch.equal(torch.floor(torch.log2(m)), (torch.frexp(m)[1] - 1).to(m.dtype))


def _assert_spread(w):
    """(ii): the non-zero magnitudes over the 27 taps of every (output, input) pair -- which hold every 3-term and every 8-term sum -- within 2^24"""
    a = w.reshape(w.shape[0], w.shape[1], 27).abs().double()
    hi, lo = a.amax(dim=2), torch.where(a > 0, a, torch.full_like(a, float("inf"))).amin(dim=2)
    assert bool(((hi == 0) | (hi <= lo * 2.0 ** 24)).all())


def _wino_row_max(w):
    w = w.double()
    u = torch.stack((w[..., 0], 0.5 * (w[..., 0] + w[..., 1] + w[..., 2]), 0.5 * (w[..., 0] - w[..., 1] + w[..., 2]), w[..., 2]), dim=-1)
    return u.reshape(w.shape[0], -1).abs().amax(dim=1)


def _same(dev_pack, host_pack, mode):
    assert dev_pack.mode == host_pack.mode == mode
    assert dev_pack.tensor.dtype == torch.int16 and dev_pack.tensor.is_cuda and dev_pack.out_scale.is_cuda
    assert torch.equal(dev_pack.tensor.cpu(), host_pack.tensor.cpu()), "pack bits"
    assert torch.equal(dev_pack.out_scale.cpu(), host_pack.out_scale.cpu()), "out_scale"


# ------------------------------------------------------------------------------------------------ 1. bit equality with the host builders
@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("shape", sorted(PLAIN))
def test_direct_and_winograd_packs_are_the_hosts_bits(shape, kind):
    cout, cin = PLAIN[shape]
    w = weights(cout, cin, kind)
    _assert_exponent_rule(w.reshape(cout, -1).abs().amax(dim=1))
    _assert_exponent_rule(_wino_row_max(w))
    _assert_spread(w)
    wd = w.to(DEV)
    for name, mode in MODES.items():
        _same(ops.pack_conv_weight_split_device(wd, mode), ops.pack_conv_weight_split(w, mode), mode)
    host = ops.pack_conv_weight_split_wino(w)
    _same(ops.pack_conv_weight_split_wino_device(wd), host, SPLIT_F16X2)
    if kind == "zero_row":
        assert float(host.out_scale[ZERO_ROW]) == 1.0
    if kind == "pow2_row":
        assert float(host.out_scale[POW2_ROW]) == 2.0 ** -3 and float(ops.pack_conv_weight_split(w, SPLIT_F16X2).out_scale[POW2_ROW]) == 2.0 ** -3
    if kind == "tiny_elements":
        p2 = ops.pack_conv_weight_split(w, SPLIT_F16X2).tensor[:cin // 16 * 27].reshape(-1, cout // 32, 2, 512)[:, :, 1].cpu().int()
        assert bool((((p2 & 0x7C00) == 0) & ((p2 & 0x03FF) != 0)).any()), "no subnormal second plane in this set"


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("shape", sorted(POLY))
def test_polyphase_pack_is_the_hosts_bits(shape, kind):
    cout, c0, c1 = POLY[shape]
    w = weights(cout, c0 + c1, kind, c0)
    _assert_spread(w)
    w0, wm, _ = ops.polyphase_weights(w, c0)
    assert torch.equal(w0, w[:, :c0])
    taps = torch.stack([wm[c * cout:(c + 1) * cout, :, (c >> 2):(c >> 2) + 2, ((c >> 1) & 1):((c >> 1) & 1) + 2, (c & 1):(c & 1) + 2] for c in range(8)])
    merged_max = taps.reshape(8, cout, -1).abs().amax(dim=2)                     # [class][n]: what pack_upconv_weight takes the log2 of
    _assert_exponent_rule(merged_max)
    wd = w.to(DEV)
    for mode in (SPLIT_F16X2, SPLIT_BF16X2):
        host = ops.pack_upconv_weight(wm, cout, mode)
        _same(ops.pack_upconv_weight_device(wd, c0, mode), host, mode)
    host = ops.pack_upconv_weight(wm, cout, SPLIT_F16X2)
    if kind == "zero_row":
        assert bool((host.out_scale.view(8, cout)[:, ZERO_ROW] == 1.0).all())
    if kind == "pow2_row":
        assert float(merged_max[0, POW2_ROW]) == 2.0 ** -3 and float(host.out_scale[POW2_ROW]) == 2.0 ** -3
    # the full-resolution part [0, c0) of the same weight, packed in place
    _assert_exponent_rule(w0.reshape(cout, -1).abs().amax(dim=1))
    _assert_exponent_rule(_wino_row_max(w0))
    for mode in MODES.values():
        _same(ops.pack_conv_weight_split_device(wd, mode, 0, c0), ops.pack_conv_weight_split(w0.contiguous(), mode), mode)
    _same(ops.pack_conv_weight_split_wino_device(wd, 0, c0), ops.pack_conv_weight_split_wino(w0.contiguous()), SPLIT_F16X2)


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("case", sorted(RANGES))
def test_channel_range_packs_are_the_hosts_bits_of_the_slice(case, kind):
    shape, c_lo, c_n = RANGES[case]
    cout, cin = PLAIN[shape]
    w = weights(cout, cin, kind)
    part = w[:, c_lo:c_lo + c_n].contiguous()
    _assert_exponent_rule(part.reshape(cout, -1).abs().amax(dim=1))
    _assert_exponent_rule(_wino_row_max(part))
    _assert_spread(part)
    wd = w.to(DEV)
    for mode in MODES.values():
        _same(ops.pack_conv_weight_split_device(wd, mode, c_lo, c_n), ops.pack_conv_weight_split(part, mode), mode)
    _same(ops.pack_conv_weight_split_wino_device(wd, c_lo, c_n), ops.pack_conv_weight_split_wino(part), SPLIT_F16X2)


# ------------------------------------------------------------------------------------------------ 2. the scale rule where the host's log2 rounds up
def test_scale_rule_just_below_a_power_of_two():
    """rows 0 / 1: maximum nextafter(2^-4, 0) / nextafter(2^-10, 0).  Every other element is an 8-bit integer times a power of two at least 2^-9 of its
    row's scale, so two fp16 planes hold every weight exactly (the maxima: 2 - 2^-23 = fp16(2) + a subnormal second plane)"""
    cout, cin = 32, 16
    g = torch.Generator().manual_seed(5)
    w = torch.randint(-127, 128, (cout, cin, 3, 3, 3), generator=g).float() * 2.0 ** -13
    w[1] *= 2.0 ** -6
    edge = [torch.nextafter(torch.tensor(2.0 ** -4), torch.tensor(0.0)), torch.nextafter(torch.tensor(2.0 ** -10), torch.tensor(0.0))]
    w[0, 9, 1, 2, 0], w[1, 3, 0, 1, 2] = edge[0], -edge[1]
    m = w.reshape(cout, -1).abs().amax(dim=1)
    assert m[0] == edge[0] < 2.0 ** -4 and m[1] == edge[1] < 2.0 ** -10
    pk = ops.pack_conv_weight_split_device(w.to(DEV).contiguous(), SPLIT_F16X2)
    scale = pk.out_scale.cpu()
    assert float(scale[0]) == 2.0 ** -5 and float(scale[1]) == 2.0 ** -11
    scaled = m / scale
    assert bool(((scaled >= 1.0) & (scaled < 2.0)).all())                        # (every row of this tensor has a non-zero maximum)
    planes = pk.tensor[:cin // 16 * 27].cpu().view(torch.float16).reshape(cin // 16, 27, cout // 32, 2, 2, 32, 8).float()    # [S][tap][blk][plane][h][r][i]
    rec = (planes[:, :, :, 0] + planes[:, :, :, 1]).permute(2, 4, 0, 3, 5, 1).reshape(cout, cin, 3, 3, 3) * scale.view(-1, 1, 1, 1, 1)
    assert torch.equal(rec, w)
    assert not bool(pk.tensor[cin // 16 * 27:].any())                            # the eight zero steps


# ------------------------------------------------------------------------------------------------ 3. the layer takes them
def _layer(cin, cout, in_real=None, seed=3):
    torch.manual_seed(seed)
    conv = U.SingleConv(cin, cout)
    conv.in_real = in_real
    with torch.no_grad():
        conv.groupnorm.weight.uniform_(0.5, 1.5)
        conv.groupnorm.bias.uniform_(-0.2, 0.2)
    return conv.to(DEV).eval().requires_grad_(False)


def _volume(dims, c, seed, real=None):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn((1,) + tuple(dims) + (c,), generator=g)
    if real is not None:
        v[..., real:] = 0
    return v.to(DEV)


LAYERS = {
    # name: (real in, real out, in_real, fine dims, stored c0, coarse c1, arith, the plan's (aiw, wino, poly), the cache key of its device pack)
    "direct": (32, 32, None, (8, 8, 8), 32, 0, {}, (False, False, False), ("device", SPLIT_F16X2)),
    "polyphase_direct": (96, 32, None, (16, 16, 16), 32, 64, {}, (False, False, True), ("device", "poly", SPLIT_F16X2, 32)),
    "wino128_literal": (128, 128, None, (8, 32, 32), 128, 0, dict(affine_in_weights=False), (False, True, False), ("device", "wino")),
    "wino32": (32, 32, None, (64, 64, 64), 32, 0, {}, (False, True, False), ("device", "wino")),
    "polyphase_wino32": (96, 32, None, (64, 64, 64), 32, 64, {}, (False, True, True), ("device", "poly_wino", 32)),
    "channel_padded": (24, 24, (24,), (8, 8, 8), 32, 0, {}, (False, False, False), ("device", SPLIT_F16X2)),
}


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_layer_takes_the_device_packs(name):
    cin, cout, in_real, dims, c0, c1, kw, want, key = LAYERS[name]
    host, dev = Arith(**kw), Arith(**kw).replace(device_packs=True)
    stored_out = U.stored_channels(cout)
    plan = U.conv_plan(host, dims, c0, c1, stored_out)
    assert plan == U.conv_plan(dev, dims, c0, c1, stored_out)
    assert plan.mode == SPLIT_F16X2 and (plan.aiw, plan.wino, plan.poly) == want and plan.small == 0
    conv = _layer(cin, cout, in_real)
    src0 = _volume(dims, c0, 11, None if in_real is None else in_real[0])
    src1 = _volume([n // 2 for n in dims], c1, 12) if c1 else None

    def both():
        yd, _ = conv.run(src0, src1, arith=dev)
        assert key in conv.__dict__["_split_packs"]._items                        # the device builder's pack, under its own key
        yh, _ = conv.run(src0, src1, arith=host)
        assert torch.isfinite(yh).all() and bool((yh != 0).any())
        assert torch.equal(yd.view(torch.int32), yh.view(torch.int32))
        return yd
    y0 = both()
    with torch.no_grad():
        conv.conv.weight.mul_(1.25).add_(0.003)
    y1 = both()
    assert not torch.equal(y0, y1)


# ------------------------------------------------------------------------------------------------ 4. no host synchronisation
def test_forward_after_a_weight_update_does_not_synchronise():
    torch.manual_seed(4)
    net = U.Abstract3DUNet(in_channels=32, out_channels=16, f_maps=32, num_levels=2).to(DEV).eval().requires_grad_(False)
    x = _volume((16, 16, 16), 32, 13)
    host, dev = Arith(), Arith(device_packs=True)

    def bump():
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(1.01)
    ref = net.run(x, arith=host)                                                  # warm: everything that is built once exists
    assert torch.equal(net.run(x, arith=dev), ref)
    bump()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        y = net.run(x, arith=dev)
        bump()
        with pytest.raises(RuntimeError, match="synchroniz"):
            net.run(x, arith=host)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert not torch.equal(y, ref) and torch.isfinite(y).all()


# ------------------------------------------------------------------------------------------------ 5. training is unchanged in its bits
def _small_pipeline(seed=1):
    """the small model of tests/test_gpu_train_pipeline.py (config A), rebuilt here"""
    hp = dict(pointnet2_params=dict(feature_dim=16, batch_norm=True, dropout=False, sa1_ratio=0.5, sa1_r=0.25, sa2_ratio=0.25, sa2_r=0.5, fp3_k=1,
                                    fp2_k=3, fp1_k=3, nocs_bins=8),
              volume_agg_params=dict(nn_channels=[25, 25, 16], batch_norm=True, lower_corner=[0, 0, 0], upper_corner=[1, 1, 1], grid_shape=[8, 8, 8],
                                     reduce_method="max", include_point_feature=True, include_confidence_feature=True),
              unet3d_params=dict(in_channels=16, out_channels=16, f_maps=(16, 48), layer_order="gcr", num_groups=8, num_levels=2),
              volume_decoder_params=dict(nn_channels=[16, 32, 32, 1], batch_norm=True),
              surface_decoder_params=dict(nn_channels=[16, 32, 32, 3], batch_norm=True),
              mc_surface_decoder_params=dict(nn_channels=[16, 32, 32, 1], batch_norm=True), mc_surface_loss_weight=0.0, learning_rate=1e-3)
    model = ConvImplicitWNFPipeline(**hp)
    model.load_state_dict(synthetic.synthetic_state_dict(hp, seed, planted_nocs=True))
    sizes, g = [200, 137], torch.Generator().manual_seed(41)
    n, nb = sum(sizes), len(sizes)
    batch = Batch(sizes=sizes, x=torch.rand(n, 3, generator=g), pos=torch.rand(n, 3, generator=g), batch=torch.arange(nb).repeat_interleave(torch.tensor(sizes)),
                  volume_query_points=torch.rand(nb, 96, 3, generator=g), gt_volume_value=torch.rand(nb, 96, generator=g),
                  surf_query_points=torch.rand(nb, 80, 3, generator=g), gt_sim_points=0.3 * torch.randn(nb, 80, 3, generator=g))
    return model, batch


def test_three_training_steps_are_the_same_bits():
    start, batch = _small_pipeline()
    start, batch = start.to(DEV).requires_grad_(True).train(), batch.to(DEV)

    def run(device_packs):
        model = copy.deepcopy(start)
        model.arith = model.arith.replace(device_packs=device_packs)
        opt = model.configure_optimizers()
        return [TP.train_step(model, opt, batch)["loss"] for _ in range(3)], model
    ld, md = run(True)
    lh, mh = run(False)
    unet = md.unet_3d.abstract_3d_unet
    built = [k for m in unet.modules() if isinstance(m, U.SingleConv) for k in U.param_cache(m, "_split_packs")._items]
    assert any(isinstance(k, tuple) and k[0] == "device" for k in built)          # the step's forward did take device packs
    print(f"[weight-pack] three steps: loss {ld} (device packs), {lh} (host packs)")
    assert ld == lh and ld[0] != ld[2]
    sd, sh = md.state_dict(), mh.state_dict()
    assert set(sd) == set(sh)
    for k in sd:
        assert torch.equal(sd[k], sh[k]), k
    assert not torch.equal(sd["unet_3d.abstract_3d_unet.decoders.0.basic_module.SingleConv2.conv.weight"],
                           start.state_dict()["unet_3d.abstract_3d_unet.decoders.0.basic_module.SingleConv2.conv.weight"])
