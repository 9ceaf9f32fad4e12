"""GPU (-m gpu): every variant of the DIRECT 3x3x3 conv kernels (csrc/unet.hip, csrc/unet_split.hip) held to fp64 and to the other variants, bit for bit.

conv_plan (components/unet3d.py) never looks at the batch size; the C dispatch of the direct kernels does (conv3d_gcr_split_impl, gn_conv3d_gcr:
workgroup counts that include B), on the claim that all the variants give the same bits.  Batch-slot independence of inference, "occupancy-aware ==
dense" (the border-class constants come from a 5^3 launch, whichever variant that takes) and the f16x2 data gradient stand on that claim.  Here it is
tested directly: for a sample shape, expected_kernel -- a restatement of the C dispatch rule -- gives the smallest B at which each variant starts; the
layer is launched one below and at every such B, and a sample's output must be torch.equal between the two launches and to a B = 1 launch of that
sample alone.  gn_last_kernel() is asserted against expected_kernel after EVERY launch of the module, and every case asserts the set of names it saw.

Which case launches which gn_note_kernel name of the direct family (shapes (16, 16, 32) and the ragged (14, 12, 30): 32 tiles of 4 x 8 x 8, 16 of 8 x 8 x 8):
    conv3d_gcr_kernel<1> / <2>                 test_fp32_variants (B = 31 | 32 at Cout 64, 15 | 16 at Cout 128; one and two sources), test_bwd_data_fp32
    conv3d_split_kernel<1, 2, true / false>    test_split_variants 1src_c64 (B = 15), 1src_c128 (7), 2src_c192 (10), 2src_c128 (15); every B = 1 launch
    conv3d_split_kernel<2, 2, true / false>    test_split_variants 2src_c192 (B = 11)
    conv3d_split_kernel<1, 3, false>           test_split_variants 1src_c128 / 2src_c128 in mode 3 (B = 15)
    conv3d_split_kernel<2, 3, false>           the same (B = 16)
    conv3d_split_strip_kernel<true / false>    test_split_variants 1src_c64 (B = 16), 1src_c128 (8 and 15); test_bwd_data_split, test_persample_variants,
                                               test_occupancy_constants_cross_variant (<true> and <false>: dense and occupancy-aware at B = 8)
    conv3d_split_wide_kernel<2, true / false>  test_split_variants 1src_c128 (B = 16), 2src_c128 (16: with the upsampled source); test_bwd_data_split,
                                               test_persample_variants (<2, true>)
    with a polyphase partial, ragged tiles     test_partial_variants (14, 12, 30), 32 -> 128: <1, 2, true>, strip<true> (B = 8), wide<2, true> (16), both
                                               entries; <1, 3, false>, <2, 3, false> (16)
(gn_conv3d_gcr_split_persample is GN_SPLIT_F16X2 with one source: <1, 2, true>, strip<true> and wide<2, true> are all it can take -- with one source
the strip rule always holds before the 64-wide one.)  NOT covered: the fits32 == false branch of conv3d_gcr_split_impl (a 128-wide layer kept off
conv3d_split_wide_kernel because one sample of its source exceeds 2^32 bytes): that needs a sample above 4 GiB, which cannot be small.

What a case asserts: (a) variant against variant and against the B = 1 launch, torch.equal on the raw fp32 output, relu on and off (mode 4: with
and without a per-sample act_inv); (b) every variant against fp64 on two slots by the suite's own bars (modes 4 / 3: 2 * max(e32, 2e-6), e32 the
fp32-MFMA kernel's error on the same slots; mode 2: 2e-4; gn_conv3d_gcr: rtol 1e-4, atol 2e-5 against torch fp32); (c) the epilogue statistics
against the fp64 sums of the stored output, per sample <= 1e-9 * max(1, |largest|); (d) run-to-run bit identity.  A reorder of two tap products in any
one variant changes that variant's fp32 accumulation order and fails (a): first `assert torch.equal(out[slot], single(slot)[0])` in _variant_checks (the
B-sample launch against the B = 1 launch of the sample alone), behind it `assert torch.equal(outs[T][:T - 1], outs[T - 1])` (the launch at the threshold
against the launch one below).  Tried once on a build with two products exchanged in each of conv3d_split_strip_kernel, conv3d_split_wide_kernel,
conv3d_split_kernel<2, ...> and conv3d_gcr_kernel<2> (the <1> kernels untouched): every launching test of the module failed at that first assertion,
each of the eight non-<1> names alone in at least one case; test_bwd_data_*, test_persample_variants and the occupancy test failed as well.

Inputs: every slot another sample of a seeded generator; exact zeros and -0.0 at some voxels; slot BIG a factor 2^10 above the others; a, d rows made
on the host (both launches read the same rows -- ops.channel_stats' atomics may move their last bit between two runs).

Figures of one run on an MI355X (the `[conv-variant]` lines: per variant the largest error / its bar over relu on / off and, mode 4, act_inv on / off).
Within a case every variant printed the SAME error to the last digit -- they are bit-identical, and expected_kernel agreed with the library on every
launch.  Error against fp64 on the two reference slots, (16, 16, 32) / (14, 12, 30):
    1src_c64    f16x2 2.24e-06 / 2.28e-06 (e32 3.39e-06 / 3.07e-06: bars 6.79e-06 / 6.14e-06)    bf16x2 2.64e-05 / 2.51e-05 (bar 2e-4)
    1src_c128   f16x2 2.43e-06 / 2.18e-06 (e32 3.64e-06 / 3.97e-06)                              bf16x2 2.57e-05 / 2.61e-05
    2src_c192   f16x2 2.44e-06 / 2.12e-06 (e32 3.52e-06 / 3.27e-06)                              bf16x2 2.60e-05 / 2.52e-05
    2src_c128   f16x2 2.64e-06 / 2.26e-06 (e32 4.45e-06 / 3.39e-06)                              bf16x2 2.63e-05 / 2.59e-05
    bf16x3      1src_c128 (14, 12, 30) 3.01e-06 (e32 3.97e-06); 2src_c128 (16, 16, 32) 3.19e-06 (e32 4.45e-06)
    fp32        largest |ours - torch fp32| / (2e-5 + 1e-4 |ref|): 0.116 (32 -> 64), 0.129 (32 -> 128), 0.127 (16 + 16 -> 64), 0.136 (16 + 32 -> 128)
    statistics  largest error / (1e-9 * max(1, |largest|)) over all cases and variants: 1.00e-06 (the fp64 sums agree to ~1e-15 of the largest)
    occupancy   active tiles per garment [6, 5, 5, 6, 4, 5, 5, 0] (f16x2) / [7, 5, 4, 4, 4, 7, 5, 0] (bf16x2) of 32; constants from
                conv3d_split_kernel<1, 2, *>, launch conv3d_split_strip_kernel<*>: equal to the dense launch
The module takes about 4 s, the slowest case 1 s (the first launch of the session).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from garmentnets_amd import ops  # noqa: E402

DEV = "cuda:0"
FP32, BF16X2, BF16X3, F16X2 = ops.CONV_FP32, ops.SPLIT_BF16X2, ops.SPLIT_BF16X3, ops.SPLIT_F16X2
BIG = 2                      # the slot whose samples are 2^10 larger than the others'
B_SCAN = 64                  # thresholds are looked for in B = 1 .. B_SCAN
CUBOID, RAGGED = (16, 16, 32), (14, 12, 30)


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- 1. the C dispatch rule, restated
def expected_kernel(entry, mode, B, dims, C0, C1, Cout):
    """the name gn_note_kernel records for a DIRECT-form launch: the conditions of gn_conv3d_gcr (csrc/unet.hip) and conv3d_gcr_split_impl
    (csrc/unet_split.hip, wino == 0) restated.  entry: the C entry; mode: GN_SPLIT_* (ignored by gn_conv3d_gcr; _persample is GN_SPLIT_F16X2)"""
    D, H, W = dims
    tiles = _cdiv(D, 4) * _cdiv(H, 8) * _cdiv(W, 8)
    if entry == "gn_conv3d_gcr":
        wide = Cout % 64 == 0 and tiles * (Cout // 64) * B >= 1024
        return "conv3d_gcr_kernel<2>" if wide else "conv3d_gcr_kernel<1>"
    if entry == "gn_conv3d_gcr_split_persample":
        assert C1 == 0
        mode = F16X2
    else:
        assert entry == "gn_conv3d_gcr_split", entry
    assert mode in (BF16X2, BF16X3, F16X2)
    tiles8 = _cdiv(D, 8) * _cdiv(H, 8) * _cdiv(W, 8)
    fits32 = D * H * W * C0 * 4 < (1 << 32)
    wide128 = mode != BF16X3 and Cout % 128 == 0 and C0 + C1 <= 384 and fits32 and tiles * (Cout // 128) * B >= 512
    strip = mode != BF16X3 and not wide128 and C1 == 0 and tiles8 * (Cout // 32) * B >= 512
    wide = not wide128 and not strip and Cout % 64 == 0 and tiles * (Cout // 64) * B >= 1024
    f16 = "true" if mode == F16X2 else "false"
    if strip:
        return f"conv3d_split_strip_kernel<{f16}>"
    if wide128:
        return f"conv3d_split_wide_kernel<2, {f16}>"
    return f"conv3d_split_kernel<{2 if wide else 1}, {3 if mode == BF16X3 else 2}, {f16}>"


def variant_starts(entry, mode, dims, C0, C1, Cout):
    """[(kernel name, the smallest B at which the dispatch takes it)] in ascending B, B = 1 .. B_SCAN"""
    out = []
    for B in range(1, B_SCAN + 1):
        k = expected_kernel(entry, mode, B, dims, C0, C1, Cout)
        if not out or out[-1][0] != k:
            out.append((k, B))
    return out


def last_kernel():
    return ops._lib.load().gn_last_kernel().decode()


def test_expected_kernel_thresholds_on_the_sample_shapes():
    """the restated rule on the sample shapes: the B at which each variant starts (no launch; the launches below take their B from the same function)"""
    for dims in (CUBOID, RAGGED):
        assert _cdiv(dims[0], 4) * _cdiv(dims[1], 8) * _cdiv(dims[2], 8) == 32 and _cdiv(dims[0], 8) * _cdiv(dims[1], 8) * _cdiv(dims[2], 8) == 16
        vs = lambda mode, c0, c1, cout: variant_starts("gn_conv3d_gcr_split", mode, dims, c0, c1, cout)   # noqa: E731
        assert vs(F16X2, 32, 0, 64) == [("conv3d_split_kernel<1, 2, true>", 1), ("conv3d_split_strip_kernel<true>", 16)]
        assert vs(BF16X2, 32, 0, 128) == [("conv3d_split_kernel<1, 2, false>", 1), ("conv3d_split_strip_kernel<false>", 8), ("conv3d_split_wide_kernel<2, false>", 16)]
        assert vs(F16X2, 16, 32, 192) == [("conv3d_split_kernel<1, 2, true>", 1), ("conv3d_split_kernel<2, 2, true>", 11)]
        assert vs(F16X2, 16, 32, 128) == [("conv3d_split_kernel<1, 2, true>", 1), ("conv3d_split_wide_kernel<2, true>", 16)]
        assert vs(BF16X3, 32, 0, 128) == [("conv3d_split_kernel<1, 3, false>", 1), ("conv3d_split_kernel<2, 3, false>", 16)]
        assert variant_starts("gn_conv3d_gcr_split_persample", F16X2, dims, 32, 0, 128) == vs(F16X2, 32, 0, 128)
        assert variant_starts("gn_conv3d_gcr", FP32, dims, 32, 0, 64) == [("conv3d_gcr_kernel<1>", 1), ("conv3d_gcr_kernel<2>", 32)]
        assert variant_starts("gn_conv3d_gcr", FP32, dims, 16, 32, 128) == [("conv3d_gcr_kernel<1>", 1), ("conv3d_gcr_kernel<2>", 16)]
    # (the 5^3 volume of an occupancy-aware layer's constants: <1> at every B of this module)
    assert expected_kernel("gn_conv3d_gcr_split", F16X2, 8, (5, 5, 5), 32, 0, 128) == "conv3d_split_kernel<1, 2, true>"


# ---------------------------------------------------------------------------------------------------- inputs and references, made once
class _Case:
    """the inputs of one (C0, C1, Cout, dims): Bmax different samples, channel-last, on the host (x0, x1, w, a, d, s) and on the device (the same, g*)"""


@functools.lru_cache(maxsize=None)
def _case(C0, C1, Cout, dims, Bmax):
    D, H, W = dims
    g = torch.Generator().manual_seed(1000 * C0 + 100 * C1 + Cout + D + Bmax)
    c = _Case()
    c.C0, c.C1, c.Cout, c.dims, c.Bmax = C0, C1, Cout, dims, Bmax
    c.x0 = torch.randn(Bmax, D, H, W, C0, generator=g)
    c.x0[:, 0, 0, ::2] = 0.0                           # exact zeros and -0.0: on a face and inside
    c.x0[:, 1, 1, ::2] = -0.0
    c.x0[:, D // 2, :, W // 2, ::3] = 0.0
    c.x1 = None
    if C1:
        c.x1 = torch.randn(Bmax, D // 2, H // 2, W // 2, C1, generator=g)
        c.x1[:, 0, 0, ::2] = -0.0
        c.x1[BIG] *= 1024.0
    c.x0[BIG] *= 1024.0                                # (a power of two: the zeros stay zeros, every other value exact)
    c.w = torch.randn(Cout, C0 + C1, 3, 3, 3, generator=g) / (27 * (C0 + C1)) ** 0.5
    c.a = 0.5 + torch.rand(Bmax, C0 + C1, generator=g)
    c.d = 0.3 * torch.randn(Bmax, C0 + C1, generator=g)
    # a per-sample power-of-two activation scale for act_inv, made on the host: the largest |x * a + d| of the sample brought into [1, 2) -- an
    # upper estimate from max |x|, max a, max |d| is enough (any power of two is undone exactly)
    top = c.x0.abs().amax(dim=(1, 2, 3, 4)) if c.x1 is None else torch.maximum(c.x0.abs().amax(dim=(1, 2, 3, 4)), c.x1.abs().amax(dim=(1, 2, 3, 4)))
    c.s = torch.exp2(-torch.floor(torch.log2(top * c.a.amax(dim=1) + c.d.abs().amax(dim=1))))
    for k in ("x0", "x1", "a", "d", "s"):
        v = getattr(c, k)
        setattr(c, "g" + k, None if v is None else v.to(DEV))
    return c


def _operand(c, slot, dtype):
    """cat(x0, nearest-upsampled x1) * a + d of one slot, (1, C, D, H, W)"""
    x = c.x0[slot:slot + 1].permute(0, 4, 1, 2, 3).to(dtype)
    if c.x1 is not None:
        x = torch.cat((x, F.interpolate(c.x1[slot:slot + 1].permute(0, 4, 1, 2, 3).to(dtype), size=c.dims, mode="nearest")), dim=1)
    return x * c.a[slot].to(dtype)[None, :, None, None, None] + c.d[slot].to(dtype)[None, :, None, None, None]


@functools.lru_cache(maxsize=None)
def _ref(C0, C1, Cout, dims, Bmax, slot, dtype):
    """conv3d(cat(x0, up(x1)) * a + d, w, padding=1) of one slot on the CPU, BEFORE the ReLU, channel-last (D, H, W, Cout); computed once and left unchanged"""
    c = _case(C0, C1, Cout, dims, Bmax)
    return F.conv3d(_operand(c, slot, dtype), c.w.to(dtype), None, padding=1)[0].permute(1, 2, 3, 0).contiguous()


def _ref_of(c, slot, relu, dtype=torch.float64):
    r = _ref(c.C0, c.C1, c.Cout, c.dims, c.Bmax, slot, dtype)
    return F.relu(r) if relu else r


@functools.lru_cache(maxsize=None)
def _pack(C0, C1, Cout, dims, Bmax, mode):
    c = _case(C0, C1, Cout, dims, Bmax)
    return ops.pack_conv_weight(c.w).to(DEV) if mode == FP32 else ops.pack_conv_weight_split(c.w, mode).to(DEV)


def _pack_of(c, mode):
    return _pack(c.C0, c.C1, c.Cout, c.dims, c.Bmax, mode)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_inputs():
    yield
    for f in (_case, _ref, _pack, _e32):
        f.cache_clear()


def _launch(c, mode, lo, hi, relu, act=False, with_stats=False):
    """slots [lo, hi) of the case through gn_conv3d_gcr (mode FP32) / gn_conv3d_gcr_split, the kernel name asserted against expected_kernel -> (result, name)"""
    B = hi - lo
    x0 = c.gx0[lo:hi].contiguous()
    x1 = None if c.gx1 is None else c.gx1[lo:hi].contiguous()
    a, d = c.ga[lo:hi].contiguous(), c.gd[lo:hi].contiguous()
    if mode == FP32:
        assert not act
        r = ops.conv3d_gcr(x0, x1, a, d, _pack_of(c, mode), c.Cout, relu=relu, with_stats=with_stats)
        want = expected_kernel("gn_conv3d_gcr", mode, B, c.dims, c.C0, c.C1, c.Cout)
    else:
        inv = None
        if act:
            s = c.gs[lo:hi]
            a, d, inv = (a * s[:, None]).contiguous(), (d * s[:, None]).contiguous(), (1.0 / s).contiguous()
        r = ops.conv3d_gcr_split(x0, x1, a, d, _pack_of(c, mode), c.Cout, relu=relu, with_stats=with_stats, act_inv=inv)
        want = expected_kernel("gn_conv3d_gcr_split", mode, B, c.dims, c.C0, c.C1, c.Cout)
    name = last_kernel()
    assert name == want, (name, want, B)
    return r, name


@functools.lru_cache(maxsize=None)
def _e32(C0, C1, Cout, dims, Bmax, slots, relu):
    """the fp32-MFMA kernel's own error against fp64 on the reference slots of the case (the yardstick of the f16x2 / bf16x3 contract)"""
    c = _case(C0, C1, Cout, dims, Bmax)
    return max(float((_launch(c, FP32, s, s + 1, relu)[0][0].cpu().double() - _ref_of(c, s, relu)).abs().max()) for s in slots)


def _stats_figure(out, s, q):
    """the epilogue statistics against the fp64 sums of the stored output: the largest error / (1e-9 * max(1, |largest|)) over the samples, each
    sample by its own largest entry (test_conv3d_winograd_against_fp64's rule, per sample: the slot 2^10 above the others does not widen theirs)"""
    o = out.double()
    worst = 0.0
    for got, want in ((s, o.sum(dim=(1, 2, 3))), (q, (o * o).sum(dim=(1, 2, 3)))):
        bound = 1e-9 * got.abs().amax(dim=1).clamp_min(1.0)
        worst = max(worst, float(((got - want).abs().amax(dim=1) / bound).max()))
    return worst


def _variant_checks(c, mode, names, relu, act, figs, seen):
    """one (relu, act_inv) setting of a case: launches one below and at every variant threshold; 3(a), (c), (d) asserted here, the figures of (b), (c)
    collected into figs[name] = [(what, value, bar)] for the caller to print before it asserts them"""
    entry = "gn_conv3d_gcr" if mode == FP32 else "gn_conv3d_gcr_split"
    starts = variant_starts(entry, mode, c.dims, c.C0, c.C1, c.Cout)
    assert [k for k, _ in starts] == list(names), (starts, names)            # the case's variants, in this order, and no other
    thresholds = [T for _, T in starts[1:]]
    assert thresholds and thresholds[-1] <= c.Bmax
    sizes = sorted({T - 1 for T in thresholds} | set(thresholds))
    ref_slots = (0, sizes[0] - 1)                                            # in every launch of the case; never the large slot
    assert BIG not in ref_slots and BIG < sizes[0]
    singles = {}

    def single(slot):
        if slot not in singles:
            singles[slot], k1 = _launch(c, mode, slot, slot + 1, relu, act)
            assert k1 == starts[0][0]
            seen.add(k1)
        return singles[slot]
    outs, kern = {}, {}
    for B in sizes:
        (out, (s, q, V)), name = _launch(c, mode, 0, B, relu, act, with_stats=True)
        assert V == c.dims[0] * c.dims[1] * c.dims[2]
        seen.add(name)
        outs[B], kern[B] = out, name
        # (d) run to run, and with the statistics off
        again, _ = _launch(c, mode, 0, B, relu, act)
        assert torch.equal(out, again), (name, B, "run to run")
        # (a) against the B = 1 launch of the sample alone
        for slot in sorted({0, B - 1, B // 2, BIG}):
            assert torch.equal(out[slot], single(slot)[0]), (name, B, slot, "against the B = 1 launch")
        # (c)
        figs.setdefault(name, []).append(("stats", _stats_figure(out, s, q), 1.0))
        # (b)
        for slot in ref_slots:
            got = out[slot].cpu()
            if mode == FP32:
                ref32 = _ref_of(c, slot, relu, torch.float32)
                figs[name].append(("fp32", float(((got - ref32).abs() / (2e-5 + 1e-4 * ref32.abs())).max()), 1.0))
            else:
                err = float((got.double() - _ref_of(c, slot, relu)).abs().max())
                e32 = _e32(c.C0, c.C1, c.Cout, c.dims, c.Bmax, ref_slots, relu)
                figs[name].append((f"fp64 (e32 {e32:.2e})", err, 2e-4 if mode == BF16X2 else 2 * max(e32, 2e-6)))
    # (a) variant against variant: the launch at the threshold against the launch one below, every slot they share
    for (name, T), (below, _) in zip(starts[1:], starts[:-1]):
        assert kern[T] == name and kern[T - 1] == below and name != below
        assert torch.equal(outs[T][:T - 1], outs[T - 1]), (name, below, T, "variant against variant")


def _report_and_assert(tag, figs, seen, names):
    line = []
    for name, items in figs.items():
        worst = {}
        for what, value, bar in items:
            key = what.split(" ")[0]
            if key not in worst or value / bar > worst[key][0] / worst[key][1]:
                worst[key] = (value, bar, what)
        line.append(name + ": " + ", ".join(f"{w} {v:.2e} / {b:.2e}" for v, b, w in worst.values()))
    print(f"[conv-variant] {tag}: " + "; ".join(line))
    assert seen == set(names), (seen, names)                                  # a silent fall into one variant fails here
    for name, items in figs.items():
        for what, value, bar in items:
            assert value <= bar, (tag, name, what, value, bar)


def _k(nt, mode):
    return f"conv3d_split_kernel<{nt}, {3 if mode == BF16X3 else 2}, {'true' if mode == F16X2 else 'false'}>"


def _strip(mode):
    return f"conv3d_split_strip_kernel<{'true' if mode == F16X2 else 'false'}>"


def _wide(mode):
    return f"conv3d_split_wide_kernel<2, {'true' if mode == F16X2 else 'false'}>"


# ---------------------------------------------------------------------------------------------------- 2. + 3. the cases
SPLIT_CASES = {
    #            C0  C1  Cout  variants in ascending B
    "1src_c64": (32, 0, 64, lambda m: (_k(1, m), _strip(m))),
    "1src_c128": (32, 0, 128, lambda m: (_k(1, m), _strip(m), _wide(m))),
    "2src_c192": (16, 32, 192, lambda m: (_k(1, m), _k(2, m))),
    "2src_c128": (16, 32, 128, lambda m: (_k(1, m), _wide(m))),
}
MODE3_CASES = {"1src_c128": (32, 0, 128), "2src_c128": (16, 32, 128)}


@pytest.mark.parametrize("dims", [CUBOID, RAGGED], ids=["16x16x32", "14x12x30"])
@pytest.mark.parametrize("mode", [F16X2, BF16X2], ids=["f16x2", "bf16x2"])
@pytest.mark.parametrize("case", list(SPLIT_CASES))
def test_split_variants(case, mode, dims):
    """gn_conv3d_gcr_split, two-plane modes: every variant one below and at its threshold (module docstring)"""
    C0, C1, Cout, names = SPLIT_CASES[case]
    names = names(mode)
    c = _case(C0, C1, Cout, dims, 16)
    figs, seen = {}, set()
    for act in ((False, True) if mode == F16X2 else (False,)):
        for relu in (True, False):
            _variant_checks(c, mode, names, relu, act, figs, seen)
    _report_and_assert(f"split {case} mode {mode} {dims}", figs, seen, names)


@pytest.mark.parametrize("case,dims", [("1src_c128", RAGGED), ("2src_c128", CUBOID)])
def test_split_variants_bf16x3(case, dims):
    """mode 3 (three bf16 planes) takes conv3d_split_kernel alone: <1, 3, false> below, <2, 3, false> from 1024 workgroups of 64 columns on"""
    C0, C1, Cout = MODE3_CASES[case]
    names = (_k(1, BF16X3), _k(2, BF16X3))
    c = _case(C0, C1, Cout, dims, 16)
    figs, seen = {}, set()
    for relu in (True, False):
        _variant_checks(c, BF16X3, names, relu, False, figs, seen)
    _report_and_assert(f"split {case} mode 3 {dims}", figs, seen, names)


@pytest.mark.parametrize("C0,C1,Cout,dims", [(32, 0, 64, RAGGED), (32, 0, 128, CUBOID), (16, 16, 64, CUBOID), (16, 32, 128, RAGGED)])
def test_fp32_variants(C0, C1, Cout, dims):
    """gn_conv3d_gcr (fp32 MFMA): <1> below, <2> from tiles * (Cout / 64) * B >= 1024 on -- conv_plan returns the fp32 plan without looking at B either"""
    names = ("conv3d_gcr_kernel<1>", "conv3d_gcr_kernel<2>")
    c = _case(C0, C1, Cout, dims, 1024 // (32 * (Cout // 64)))
    figs, seen = {}, set()
    for relu in (True, False):
        _variant_checks(c, FP32, names, relu, False, figs, seen)
    _report_and_assert(f"fp32 {C0}+{C1}->{Cout} {dims}", figs, seen, names)


# ---------------------------------------------------------------------------------------------------- 4. the same promise where it is used
def _grad_case(cout_layer, cin_p, dims, Bmax):
    """a masked output gradient [Bmax][D][H][W][cout_layer] (zeros where the ReLU was off, slot BIG 2^10 larger) and a layer weight (cout_layer, cin_p, 3, 3, 3)"""
    g = torch.Generator().manual_seed(cout_layer + cin_p + dims[0])
    dy = torch.randn(Bmax, *dims, cout_layer, generator=g)
    dy = dy * (torch.rand(Bmax, *dims, cout_layer, generator=g) < 0.6)
    dy[:, 1, 1, ::2] = -0.0
    dy[BIG] *= 1024.0
    w = torch.randn(cout_layer, cin_p, 3, 3, 3, generator=g) / (27 * cin_p) ** 0.5
    return dy.to(DEV), w


def _slot_independent(call, entry, mode, dims, C0, Cout, names):
    """call(lo, hi) -> the op over slots [lo, hi): one below and at every threshold, each B-sample call against the single-sample calls and the call below"""
    starts = variant_starts(entry, mode, dims, C0, 0, Cout)
    assert [k for k, _ in starts] == list(names), (starts, names)
    seen, outs, singles = set(), {}, {}
    for B in sorted({T - 1 for _, T in starts[1:]} | {T for _, T in starts[1:]}):
        outs[B] = call(0, B)
        name = last_kernel()
        assert name == expected_kernel(entry, mode, B, dims, C0, 0, Cout), (name, B)
        seen.add(name)
        assert torch.equal(outs[B], call(0, B))
        for slot in sorted({0, B - 1, B // 2, BIG}):
            if slot not in singles:
                singles[slot] = call(slot, slot + 1)
                assert last_kernel() == starts[0][0]
                seen.add(starts[0][0])
            assert torch.equal(outs[B][slot], singles[slot][0]), (name, B, slot)
    for _, T in starts[1:]:
        assert torch.equal(outs[T][:T - 1], outs[T - 1]), T
    assert seen == set(names), (seen, names)


@pytest.mark.parametrize("dims", [CUBOID, RAGGED], ids=["16x16x32", "14x12x30"])
def test_bwd_data_split(dims):
    """ops.conv3d_bwd_data_split (gn_conv3d_gcr_split on the transposed pack, 32 -> 128: <1>, strip, 128-wide): sample b's gradient from the B-sample call
    == the call on g[b:b+1], scale[b:b+1], inv[b:b+1]"""
    cout_layer, cin_p = 32, 128
    g, w = _grad_case(cout_layer, cin_p, dims, 16)
    pack = ops.pack_conv_weight_bwd_data_split(w).to(DEV)
    s = torch.exp2(-torch.floor(torch.log2(g.abs().amax(dim=(1, 2, 3, 4)))))           # relu_mask_max's kind of scale: a power of two per sample
    scale, inv = s[:, None].expand(-1, cout_layer).contiguous(), (1.0 / s).contiguous()
    call = lambda lo, hi: ops.conv3d_bwd_data_split(g[lo:hi].contiguous(), scale[lo:hi].contiguous(), inv[lo:hi].contiguous(), pack, cin_p)   # noqa: E731
    _slot_independent(call, "gn_conv3d_gcr_split", F16X2, dims, cout_layer, cin_p, (_k(1, F16X2), _strip(F16X2), _wide(F16X2)))


def test_bwd_data_fp32():
    """ops.conv3d_bwd_data (gn_conv3d_gcr on the transposed pack, 32 -> 128) across <1> / <2>"""
    cout_layer, cin_p, dims = 32, 128, RAGGED
    g, w = _grad_case(cout_layer, cin_p, dims, 16)
    wp = ops.pack_conv_weight_bwd_data(w).to(DEV)
    _slot_independent(lambda lo, hi: ops.conv3d_bwd_data(g[lo:hi].contiguous(), wp, cin_p), "gn_conv3d_gcr", FP32, dims, cout_layer, cin_p,
                      ("conv3d_gcr_kernel<1>", "conv3d_gcr_kernel<2>"))


@pytest.mark.parametrize("dims", [CUBOID, RAGGED], ids=["16x16x32", "14x12x30"])
def test_persample_variants(dims):
    """the affine-in-weights form (ops.conv_affine_pack + ops.conv3d_gcr_split_persample, 32 -> 128): sample b's pack, scales and bias table do not depend on
    the batch it was built in, and its output is the same through <1>, strip and the 128-wide kernel.  Statistics rows made on the host (fp64 sums)"""
    c = _case(32, 0, 128, dims, 16)
    w = c.w.to(DEV).contiguous()
    V = dims[0] * dims[1] * dims[2]
    sm, sq = c.x0.double().sum(dim=(1, 2, 3)).to(DEV), (c.x0.double() ** 2).sum(dim=(1, 2, 3)).to(DEV)
    per = (c.C0 // 16) * 27 * (c.Cout // 32) * 2 * 1024                                 # bytes of one sample's pack

    @functools.lru_cache(maxsize=None)
    def prep(lo, hi):
        return ops.conv_affine_pack(w, c.ga[lo:hi].contiguous(), c.gd[lo:hi].contiguous(), (sm[lo:hi].contiguous(), sq[lo:hi].contiguous(), V))
    full = prep(0, 16)
    for b in (0, BIG, 7, 15):
        one = prep(b, b + 1)
        assert torch.equal(full.pack[b * per:(b + 1) * per], one.pack[:per]), ("pack bytes", b)
        assert torch.equal(full.out_scale[b], one.out_scale[0]) and torch.equal(full.kbias[b], one.kbias[0]), ("scales / bias table", b)
        assert torch.equal(full.stage_a[b], one.stage_a[0]) and torch.equal(full.stage_d[b], one.stage_d[0]), ("staging affine", b)
    for B in (7, 8, 15):
        part = prep(0, B)
        assert torch.equal(full.pack[:B * per], part.pack[:B * per]) and torch.equal(full.out_scale[:B], part.out_scale) and torch.equal(full.kbias[:B], part.kbias)
    for relu in (True, False):
        call = lambda lo, hi: ops.conv3d_gcr_split_persample(c.gx0[lo:hi].contiguous(), prep(lo, hi), relu=relu)   # noqa: E731,B023
        _slot_independent(call, "gn_conv3d_gcr_split_persample", F16X2, dims, c.C0, c.Cout, (_k(1, F16X2), _strip(F16X2), _wide(F16X2)))


def _upsampled_partial(part, dims):
    """partial [B][D/2][H/2][W/2][8 * Cout] -> what the epilogue adds at every voxel, [B][D][H][W][Cout]: entry ((z&1)*4 + (y&1)*2 + (x&1)) * Cout + n
    of coarse voxel (z>>1, y>>1, x>>1)"""
    B, (D, H, W) = part.shape[0], dims
    return part.view(B, D // 2, H // 2, W // 2, 2, 2, 2, -1).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, D, H, W, -1)


@pytest.mark.parametrize("mode", [F16X2, BF16X3], ids=["f16x2", "bf16x3"])
def test_partial_variants(mode):
    """a polyphase partial on RAGGED tiles through every direct split variant (32 -> 128 at (14, 12, 30)): <1, 2, true>, strip, 128-wide (f16x2) and
    <1, 3, false>, <2, 3, false> (bf16x3).  Every variant one below and at its threshold, bit for bit and against its B = 1 launch (_slot_independent);
    each variant against fp64 (the conv reference + the partial, added before the ReLU; the bars of _variant_checks) with its epilogue statistics; the
    f16x2 case through the affine-in-weights entry as well (kbias and partial together).  The partial enters by ONE __fadd_rn before the ReLU, so
    the launch with it must also equal the launch without it (relu off) + partial, then ReLU, to the bit."""
    C0, Cout, dims, Bmax = 32, 128, RAGGED, 16
    names = (_k(1, mode), _strip(mode), _wide(mode)) if mode == F16X2 else (_k(1, mode), _k(2, mode))
    c = _case(C0, 0, Cout, dims, Bmax)
    D, H, W = dims
    part = torch.randn(Bmax, D // 2, H // 2, W // 2, 8 * Cout, generator=torch.Generator().manual_seed(4242 + mode))
    part[BIG] *= 1024.0
    gpart = part.to(DEV)
    up = _upsampled_partial(part, dims)                                    # host, fp32
    pack = _pack_of(c, mode)
    starts = variant_starts("gn_conv3d_gcr_split", mode, dims, C0, 0, Cout)
    assert [k for k, _ in starts] == list(names) and starts[-1][1] <= Bmax, starts
    ref_slots = (0, starts[1][1] - 2)                                      # in every launch below; never the large slot
    assert BIG not in ref_slots
    figs = {}
    for relu in (True, False):
        launch = lambda lo, hi, **kw: ops.conv3d_gcr_split(c.gx0[lo:hi].contiguous(), None, c.ga[lo:hi].contiguous(), c.gd[lo:hi].contiguous(), pack,   # noqa: E731,B023
                                                           Cout, relu=relu, partial=gpart[lo:hi].contiguous(), **kw)                              # noqa: B023
        _slot_independent(launch, "gn_conv3d_gcr_split", mode, dims, C0, Cout, names)
        e32 = _e32(C0, 0, Cout, dims, Bmax, ref_slots, relu)
        for (name, T), B in zip(starts, [starts[1][1] - 1] + [T for _, T in starts[1:]]):
            out, (s, q, V) = launch(0, B, with_stats=True)
            assert last_kernel() == name and V == D * H * W, (last_kernel(), name, B)
            figs.setdefault(name, []).append(("stats", _stats_figure(out, s, q), 1.0))
            for slot in ref_slots:
                want = _ref_of(c, slot, False) + up[slot].double()
                err = float((out[slot].cpu().double() - (F.relu(want) if relu else want)).abs().max())
                figs[name].append((f"fp64 (e32 {e32:.2e})", err, 2 * max(e32, 2e-6)))
            # the partial is one fp32 addition before the ReLU
            bare = ops.conv3d_gcr_split(c.gx0[:B].contiguous(), None, c.ga[:B].contiguous(), c.gd[:B].contiguous(), pack, Cout, relu=False)
            assert last_kernel() == name
            want = bare + _upsampled_partial(gpart[:B], dims)
            assert torch.equal(out, F.relu(want) if relu else want), (name, B, relu, "partial added before the ReLU")
    _report_and_assert(f"partial mode {mode} {dims}", figs, set(names), names)
    if mode != F16X2:
        return
    # kbias and partial together: the affine-in-weights form of the same layer
    w = c.w.to(DEV).contiguous()
    sm, sq = c.x0.double().sum(dim=(1, 2, 3)).to(DEV), (c.x0.double() ** 2).sum(dim=(1, 2, 3)).to(DEV)

    @functools.lru_cache(maxsize=None)
    def prep(lo, hi):
        return ops.conv_affine_pack(w, c.ga[lo:hi].contiguous(), c.gd[lo:hi].contiguous(), (sm[lo:hi].contiguous(), sq[lo:hi].contiguous(), D * H * W))
    for relu in (True, False):
        call = lambda lo, hi: ops.conv3d_gcr_split_persample(c.gx0[lo:hi].contiguous(), prep(lo, hi), relu=relu, partial=gpart[lo:hi].contiguous())   # noqa: E731,B023
        _slot_independent(call, "gn_conv3d_gcr_split_persample", F16X2, dims, C0, Cout, names)
        for name, B in zip(names, [starts[1][1] - 1] + [T for _, T in starts[1:]]):
            out, (s, q, _) = ops.conv3d_gcr_split_persample(c.gx0[:B].contiguous(), prep(0, B), relu=relu, with_stats=True, partial=gpart[:B].contiguous())
            assert last_kernel() == name
            assert _stats_figure(out, s, q) <= 1.0, (name, B, "statistics")
            want = ops.conv3d_gcr_split_persample(c.gx0[:B].contiguous(), prep(0, B), relu=False) + _upsampled_partial(gpart[:B], dims)
            assert torch.equal(out, F.relu(want) if relu else want), (name, B, relu, "kbias, then the partial, then the ReLU")


@pytest.mark.parametrize("mode", [F16X2, BF16X2], ids=["f16x2", "bf16x2"])
def test_occupancy_constants_cross_variant(mode):
    """an occupancy-aware launch whose dense form takes the x-strip kernel (32 -> 128 at (16, 16, 32), B = 8) while the 5^3 launch that supplies its
    border-class constants takes conv3d_split_kernel<1>: equal to the dense launch, bit for bit -- the cross-variant dependence the comment in
    conv3d_gcr_split_impl describes.  (The pipeline path: test_sparse_first_conv_is_bit_identical_to_dense.)"""
    from garmentnets_amd.components.unet3d import _class_constants
    B, C0, Cout, dims = 8, 32, 128, CUBOID
    D, H, W = dims
    g = torch.Generator().manual_seed(77 + mode)
    x = torch.zeros(B, D, H, W, C0)
    flat = []
    for b in range(B - 1):                                                 # the last garment has no point
        n = 3 if b else 5
        cells = torch.stack([torch.randint(0, D, (n,), generator=g), torch.randint(0, H, (n,), generator=g), torch.randint(0, W, (n,), generator=g)], 1)
        if b == 0:
            cells[0], cells[1], cells[2] = torch.tensor([0, 0, 0]), torch.tensor([D - 1, H - 1, W - 1]), torch.tensor([0, H - 1, 5])
        x[b, cells[:, 0], cells[:, 1], cells[:, 2]] = torch.randn(n, C0, generator=g).abs() * 3.0
        flat.append(((b * D + cells[:, 0]) * H + cells[:, 1]) * W + cells[:, 2])
    flat = torch.cat(flat).to(torch.int32).to(DEV)
    w = torch.randn(Cout, C0, 3, 3, 3, generator=g) / (27 * C0) ** 0.5
    a, d = (0.5 + torch.rand(B, C0, generator=g)).to(DEV), (0.3 * torch.randn(B, C0, generator=g)).to(DEV)
    inv = None
    if mode == F16X2:
        s = torch.exp2(-torch.arange(B, dtype=torch.float32) % 3).to(DEV)
        a, d, inv = (a * s[:, None]).contiguous(), (d * s[:, None]).contiguous(), (1.0 / s).contiguous()
    pack = ops.pack_conv_weight_split(w, mode).to(DEV)
    xg = x.to(DEV)
    launch = lambda v, **kw: ops.conv3d_gcr_split(v, None, a, d, pack, Cout, relu=True, act_inv=inv, **kw)   # noqa: E731
    small = launch(torch.zeros((B, 5, 5, 5, C0), dtype=torch.float32, device=DEV))
    k_small = last_kernel()
    dense, (s_d, q_d, _) = launch(xg, with_stats=True)
    k_dense = last_kernel()
    flags = ops.grid_tile_flags(flat, B, dims, 1)
    occ, (s_o, q_o, _) = launch(xg, with_stats=True, tile_active=flags, kconst=_class_constants(small, 1, Cout), kreach=1)
    k_occ = last_kernel()
    assert k_small == expected_kernel("gn_conv3d_gcr_split", mode, B, (5, 5, 5), C0, 0, Cout) == _k(1, mode)
    assert k_dense == k_occ == expected_kernel("gn_conv3d_gcr_split", mode, B, dims, C0, 0, Cout) == _strip(mode)
    active = flags.sum(dim=1).tolist()
    print(f"[conv-variant] occupancy mode {mode}: active tiles per garment {active} of {flags.shape[1]}; constants from {k_small}, launch {k_occ}")
    assert active[B - 1] == 0 and 0 < min(active[:B - 1]) and max(active) < flags.shape[1]
    assert torch.equal(occ, dense)
    for got, want in ((s_o, s_d), (q_o, q_d)):                             # (the statistics up to the order of their fp64 atomics, as sparse_first_conv_case)
        assert float(((got - want).abs() / want.abs().clamp_min(1e-30)).max()) <= 1e-13
