"""3-D UNet (GroupNorm -> Conv3d -> ReLU double convs, max-pool encoder, nearest-upsample + concat decoder) on HIP.

Checkpoint-schema twin of the subset of /root/reference/components/unet3d.py that the pipeline instantiates
(``Abstract3DUNet`` with ``basic_module=DoubleConv``, ``layer_order='gcr'``): module / parameter names
``encoders.{i}.basic_module.SingleConv{1,2}.{groupnorm,conv}``, ``decoders.{i}...``, ``final_conv`` are kept.
The torch layers only hold parameters.  Execution is channel-last ([B][D][H][W][C]):
    GroupNorm  = gn_channel_stats (+ gn_groupnorm_affine)  -> per-(sample, channel) affine
    conv+ReLU  = gn_conv3d_gcr: the affine is applied while the input halo is staged into LDS, the 3x3x3 conv runs as
                 an implicit GEMM on fp32 MFMA; nearest upsampling and torch.cat((skip, x)) of the decoder
                 (components/unet3d.py:291,330) are folded into the loader (second source read at half resolution)
    MaxPool3d  = gn_maxpool3d_2,   final 1x1x1 conv = gn_linear.
"""
import functools
from typing import NamedTuple, Optional

import torch
from torch import nn

from .. import arith as AR
from .. import ops
from .mlp import PackedModule, generation, pack_wb, param_cache


def number_of_features_per_level(init_channel_number, num_levels):
    return [init_channel_number * 2 ** k for k in range(num_levels)]


# Channel padding.  The conv kernels take Cout % 32 == 0 (and Cin % 16 == 0 per source), so a layer of c output channels is STORED with
# round_up(c, 32): its weights get zero rows / columns for the pad channels, its normalisation a zero affine (a = d = 0) and its conv bias a
# zero there, so the pads hold exact zeros through every layer (ReLU / LeakyReLU / ELU of 0 is 0, and so is every border-class constant of
# the occupancy-aware launch).  A layer whose channels need no padding runs exactly the unpadded code.
CHANNEL_GRANULE = 32


def stored_channels(c):
    """the stored width of a UNet activation with c real channels"""
    return -(-int(c) // CHANNEL_GRANULE) * CHANNEL_GRANULE


class _Layout(tuple):
    """(real, stored, cout): the real and stored channel count of each source of one SingleConv call and its stored output width"""
    real = property(lambda self: self[0])
    stored = property(lambda self: self[1])
    cout = property(lambda self: self[2])


def to_stored(v, real, stored):
    """[..., sum(real)] -> [..., sum(stored)]: each source's real channels at the head of its stored block, zeros on the pads"""
    if tuple(real) == tuple(stored):
        return v
    out = v.new_zeros(tuple(v.shape[:-1]) + (sum(stored),))
    o = k = 0
    for r, st in zip(real, stored):
        out[..., o:o + r] = v[..., k:k + r]
        o, k = o + st, k + r
    return out


class AtRest(NamedTuple):
    """what is known about a layer's src0 behind gn_grid_scatter's volume: away from the scattered cells it holds one value per (sample, channel)"""
    flat: Optional[torch.Tensor]         # flat cell index of every scattered point; None: the cells are not known (no occupancy-aware launch)
    reach: int                           # 1: src0 IS the scattered volume; 2: the output of the reach-1 layer (non-constant within one voxel of the cells)
    value: Optional[torch.Tensor] = None  # [B][C0] the value at rest; None: zero at reach 1 (the scattered volume itself), not known behind it
    small: Optional[torch.Tensor] = None  # (reach 2) the reach-1 layer's output over its small all-at-rest volume


class ConvPlan(NamedTuple):
    """which launch one 3x3x3 'gcr' convolution takes (conv_plan)"""
    mode: int        # arith.conv_mode: CONV_FP32 (csrc/unet.hip) or the split-operand mode (csrc/unet_split.hip, unet_wino.hip, unet_wino32.hip)
    aiw: bool        # operand form: affine-in-weights (ops.conv_affine_pack: exact zeros where the source is at rest) instead of the literal one
    wino: bool       # kernel family: Winograd F(2,3) along x instead of direct
    poly: bool       # the upsampled source arrives as a polyphase partial (csrc/upconv.hip); the launch reads the full-resolution source alone
    small: int       # occupancy-aware launch: the edge of the small all-at-rest volume its border-class constants come from (5 or 8); 0: dense


@functools.lru_cache(maxsize=None)      # (pure, of hashable arguments: a layer's plan is decided once per shape and arithmetic, then looked up)
def conv_plan(arith, dims, c0, c1, cout, reach=0, rest_known=False, small=None, cells=False, rest0=False):
    """The launch of one 'gcr' layer as a pure function of the arithmetic, the SAMPLE's (D, H, W), the stored widths (c1 = 0: one source) and what is
    known of src0 at rest -- reach (0: nothing), rest_known (its value there), small (the dims of the previous layer's small output or None), cells
    (the scattered cells are known); rest0: a decoder's skip connection is at rest.  No tensor, no library entry, never the batch size.
    Winograd (arith.winograd: csrc/unet_wino.hip for Cout % 128 == 0; arith.winograd32: csrc/unet_wino32.hip for the 32- / 64-wide layers) is decided
    from the SAMPLE's shape alone, never from the batch size: the Winograd and the direct form round differently, and a garment's result must not
    depend on how many garments share its batch (the direct kernels may switch variant with the batch size because they are bit-identical to each other)"""
    mode, (D, H, W) = arith.conv_mode, dims
    if mode == ops.CONV_FP32:
        return ConvPlan(mode, False, False, False, 0)
    # polyphase form of a decoder's first convolution: the nearest-upsampled channels as a 2x2x2-tap convolution per output parity class on the
    # COARSE volume (8/27 of their MACs, the coarse halo staged once for all classes: csrc/upconv.hip), added in the fine launch's epilogue
    poly = c1 > 0 and arith.polyphase_upconv and mode != ops.SPLIT_BF16X3 and c1 <= 384
    # (of a polyphase layer the full-resolution part may run in Winograd form on the 32- / 64-wide layers: csrc/unet_wino32.hip takes the partial
    #  in its epilogue)
    wino = (c1 == 0 or (poly and cout % 128 != 0)) and arith.winograd and mode == ops.SPLIT_F16X2 and ops.wino_supported(c0, cout, dims)
    if wino and cout % 128 == 0:
        wino = (D // 4) * (H // 8) * (W // 8) * (cout // 128) >= 32
    elif wino:
        # the 32-wide column-block kernel (csrc/unet_wino32.hip, round 6): 8 x 8 x 8 tiles; one workgroup per CU walks chains of tiles -- worth it from a
        # few tiles per CU and sample on (the 64^3 and 128^3 levels of the UNet)
        wino = arith.winograd32 and (D // 8) * (H // 8) * (W // 8) * (cout // 32) >= 512
    # affine-in-weights: a single source at rest (0 for the scattered volume, a known value behind it), or a polyphase layer's skip connection
    aiw = arith.affine_in_weights and mode == ops.SPLIT_F16X2 and c0 % 16 == 0 and cout % 32 == 0
    aiw = aiw and ((c1 == 0 and (reach == 1 or (reach > 1 and rest_known))) or (poly and rest0))
    occ = (cells and reach > 0 and arith.sparse_first_conv and c1 == 0 and mode != ops.SPLIT_BF16X3 and c0 <= 384 and (cout % 128 == 0 or cout % 64 != 0)
           and min(dims) > 2 * reach and (reach == 1 or small is not None)
           # (a Winograd layer handed a small volume it cannot take -- 5^3, from a layer that ran in the direct form -- simply runs dense.  At reach 2
           #  the small volume holds the previous layer's face values, the operand is NOT zero there and the two forms round differently: constants
           #  from the direct pack would break "occupancy-aware == dense, bit for bit" for such mixed configurations)
           and (not wino or small is None or ops.wino_supported(c0, cout, small)))
    # (the Winograd kernels take whole tiles, 4 x 8 x 8 / 8 x 8 x 8: 8^3 is their smallest volume, 5^3 the direct kernels')
    return ConvPlan(mode, bool(aiw), bool(wino), bool(poly), (int(small[0]) if small is not None else 8 if wino else 5) if occ else 0)


class ConvGradPlan(NamedTuple):
    """which kernel each gradient of one 3x3x3 'gcr' convolution takes (conv_grad_plan): "fp32" or "f16x2" """
    data: str        # the data gradient: "fp32" gn_conv3d_gcr (csrc/unet.hip) / "f16x2" gn_conv3d_gcr_split, direct form, both on the flipped / transposed pack
    weight: str      # the weight gradient: "fp32" gn_conv3d_bwd_weight (csrc/unet_grad.hip) / "f16x2" gn_conv3d_bwd_weight_split (csrc/unet_grad_split.hip)


# The rules under which a layer's gradient stays on the fp32 kernel although arith.conv_grad_mode asks for "f16x2" -- each written here, once, by name.
def grad_data_pack_unsupported(cout_stored):
    """the data gradient reads the layer's OUTPUT width as its input, 16 channels at a time (the split pack's K slices): a stored width that is no
    multiple of 16 has no f16x2 pack (no stored activation has one -- stored_channels rounds to 32 -- but a direct caller's may)"""
    return cout_stored % 16 != 0


def grad_weight_partial_quad(c0, c1):
    """the weight gradient stages its operand four channels at a time and a quad must not straddle the two sources: both widths multiples of 4 (the
    fp32 kernel's own rule; such a layer has no weight gradient at all and the fp32 entry refuses it by name)"""
    return c0 % 4 != 0 or c1 % 4 != 0


@functools.lru_cache(maxsize=None)
def conv_grad_plan(arith, dims, c0, c1, cout_stored):
    """The backward of one 'gcr' layer as a pure function of the arithmetic, the SAMPLE's (D, H, W) and the stored widths (c1 = 0: one source): which
    kernel the data gradient and which the weight gradient takes.  No tensor, no library entry, never the batch size.  arith.conv_grad_mode "fp32":
    always the fp32 kernels.  "f16x2": the split-operand kernels unless one of the named rules above holds.  No shape rule: at both measured shapes --
    every layer of the reference's training UNet (f_maps 32, 4 levels, 32^3, down to 4^3 volumes of one tile) and 128 -> 128 at 128^3 -- the f16x2
    kernels are the faster ones (profiles/unet_grad_split_time.json, DESIGN.md "f16x2 backward of the UNet convolutions"), so dims decides nothing yet;
    it is an argument so that a measured shape rule has its place."""
    if arith.conv_grad_mode != "f16x2":
        return ConvGradPlan("fp32", "fp32")
    return ConvGradPlan("fp32" if grad_data_pack_unsupported(cout_stored) else "f16x2", "fp32" if grad_weight_partial_quad(c0, c1) else "f16x2")


_ACT = {"r": ("ReLU", lambda: nn.ReLU(inplace=True), ops.ACT_RELU), "l": ("LeakyReLU", lambda: nn.LeakyReLU(negative_slope=0.1, inplace=True), ops.ACT_LEAKY),
        "e": ("ELU", lambda: nn.ELU(inplace=True), ops.ACT_ELU)}


def _class_constants(small_out, reach, cout):
    """border-class constants of an occupancy-aware launch from the layer's output over a small all-at-rest volume (n^3, n = 5 for the direct
    kernels, 8 -- the smallest volume of whole tiles -- for the Winograd kernel): per axis the voxels at distance 0 [, 1] from either face and one
    in the middle.  (Winograd along x: voxel 0 / n-1 of the small volume has the parity of voxel 0 / W-1 of the real one, n and W being multiples
    of 8, and away from the cells both members of an output pair hold the same value -- the differences d0 - d2, d2 - d1, d1 - d3 are exactly zero.)
    Strided / indexed views of a device tensor: nothing comes from the host, the path can be captured into a HIP graph."""
    B, n = small_out.shape[0], small_out.shape[1]
    pos = [0, n // 2, n - 1] if reach == 1 else [0, 1, n // 2, n - 2, n - 1]
    k = small_out
    for dim in (1, 2, 3):                          # (narrow + cat: device-side copies only -- an index tensor would be a host-to-device copy)
        k = torch.cat([k.narrow(dim, q, 1) for q in pos], dim=dim)
    return k.reshape(B, len(pos) ** 3, cout).contiguous()


def _raw(w):
    """the weight as the device builders read it (fp32, contiguous: device-side copies when it is not)"""
    w = w.detach()
    return w if w.dtype == torch.float32 and w.is_contiguous() else w.float().contiguous()


def _host_poly(w, mode, c0):
    w0, wm, _ = ops.polyphase_weights(w, c0)
    return (ops.pack_conv_weight_split(w0, mode).to(w.device), ops.pack_upconv_weight(wm, w.shape[0], mode).to(w.device))


# Every pack of a SingleConv's convolution weight, named once: kind -> (cache key, host builder, device builder or None), each a function of
# (w: the weight in the stored layout, mode, c0).  The builders reach `ops` by name at call time.  A device pack (csrc/weight_pack.hip: no host round
# trip) sits under ("device",) + the host key, in the same ParamCache generation.
CONV_PACKS = {
    "fp32": ("fp32", lambda w, mode, c0: ops.pack_conv_weight(w), None),
    "split": (lambda mode, c0: mode, lambda w, mode, c0: ops.pack_conv_weight_split(w, mode).to(w.device),
              lambda w, mode, c0: ops.pack_conv_weight_split_device(_raw(w), mode)),
    "wino": ("wino", lambda w, mode, c0: ops.pack_conv_weight_split_wino(w).to(w.device), lambda w, mode, c0: ops.pack_conv_weight_split_wino_device(_raw(w))),
    # (full-resolution part, polyphase part) of a decoder's first convolution split at c0
    "poly": (lambda mode, c0: ("poly", mode, c0), _host_poly,
             lambda w, mode, c0: (ops.pack_conv_weight_split_device(_raw(w), mode, 0, c0), ops.pack_upconv_weight_device(_raw(w), c0, mode))),
    "poly_wino": (lambda mode, c0: ("poly_wino", c0), lambda w, mode, c0: ops.pack_conv_weight_split_wino(ops.polyphase_weights(w, c0)[0]).to(w.device),
                  lambda w, mode, c0: ops.pack_conv_weight_split_wino_device(_raw(w), 0, c0)),
    "w0": (lambda mode, c0: ("w0", c0), lambda w, mode, c0: w.detach()[:, :c0].contiguous(), None),
    # the data gradient: the forward kernels on the flipped / transposed weight
    "bwd_data": ("bwd_data", lambda w, mode, c0: ops.pack_conv_weight_bwd_data(w), None),
    "bwd_data_split": ("bwd_data_split", lambda w, mode, c0: ops.pack_conv_weight_bwd_data_split(w, False),
                       lambda w, mode, c0: ops.pack_conv_weight_bwd_data_split(w, True)),
}


class SingleConv(PackedModule, nn.Sequential):
    """One conv block of the reference's create_conv (components/unet3d.py:19-73), same module names and parameter layout for every layer order:
    'g' GroupNorm, 'b' BatchNorm3d, 'c' Conv3d 3x3x3 pad 1 (bias only when the order has no norm layer), 'r' ReLU, 'l' LeakyReLU(0.1), 'e' ELU.
    'gcr' -- what the GarmentNets pipeline ships -- runs on the fused split-operand kernels (run()); every other order ('cr', 'crg', 'cl', 'ce',
    'bcr', ...) runs the convolution on the exact fp32-MFMA kernel with the pre-conv normalisation applied on load and the rest (bias, LeakyReLU / ELU,
    a normalisation behind the non-linearity) through gn_affine_act: correct for any checkpoint, not tuned."""

    def __init__(self, in_channels, out_channels, kernel_size=3, order="gcr", num_groups=8, padding=1):
        super().__init__()
        if kernel_size != 3 or padding != 1:
            raise NotImplementedError("garmentnets_amd implements the 3x3x3, padding 1 SingleConv of the GarmentNets pipeline")
        if "c" not in order or order.count("c") != 1:
            raise ValueError("Conv layer MUST be present (exactly once)")
        if order[0] in "rle":
            raise ValueError("Non-linearity cannot be the first operation in the layer")
        if any(ch not in "bgrlec" for ch in order):
            raise ValueError(f"Unsupported layer type in {order!r}. MUST be one of ['b', 'g', 'r', 'l', 'e', 'c']")
        if any(ch in "rle" for ch in order[:order.index("c")]) or sum(ch in "gb" for ch in order[:order.index("c")]) > 1:
            raise NotImplementedError(f"layer order {order!r}: at most one normalisation and no non-linearity in front of the convolution")
        self.order = order
        # real channel count of each source when the inputs are stored channel-padded (set by DoubleConv / Decoder); None: as stored
        self.in_real = None
        for i, ch in enumerate(order):
            before = i < order.index("c")
            nch = in_channels if before else out_channels
            if ch in _ACT:
                self.add_module(_ACT[ch][0], _ACT[ch][1]())
            elif ch == "c":
                self.add_module("conv", nn.Conv3d(in_channels, out_channels, 3, padding=1, bias=not ("g" in order or "b" in order)))
            elif ch == "g":
                groups = num_groups if nch >= num_groups else 1
                assert nch % groups == 0, f"Expected number of channels in input to be divisible by num_groups. num_channels={nch}, num_groups={groups}"
                self.add_module("groupnorm", nn.GroupNorm(num_groups=groups, num_channels=nch))
            elif ch == "b":
                self.add_module("batchnorm", nn.BatchNorm3d(nch))

    def _pack(self):
        # [tap][Cin/16][Cout][16] (a layer of other widths runs channel-padded: _padded_weight)
        wp = ops.pack_conv_weight(self.conv.weight) if self.conv.in_channels % 16 == 0 else None
        gn = getattr(self, "groupnorm", None)
        return wp, (None if gn is None else gn.weight.detach().float().contiguous()), (None if gn is None else gn.bias.detach().float().contiguous())

    def _layout(self, src0, src1):
        """the channel layout of a call (_Layout), or None when nothing is padded: the unpadded code runs"""
        stored = (src0.shape[-1],) if src1 is None else (src0.shape[-1], src1.shape[-1])
        real = stored if self.in_real is None else tuple(self.in_real)
        cout = self.conv.out_channels
        if self.in_real is not None and (len(real) != len(stored) or any(r > st for r, st in zip(real, stored))):
            raise ValueError(f"SingleConv: inputs of {stored} stored channels for {real} real ones")
        if real == stored and cout % CHANNEL_GRANULE == 0:
            return None
        return _Layout((real, stored, stored_channels(cout)))

    def weight_pack(self, kind, lay, *, mode=None, c0=None, device=False):
        """The pack `kind` of the convolution weight under the channel layout `lay` (_layout: None when nothing is padded), built once per generation of
        the module's tensors and layout.  kind: "padded_weight" -- the Conv3d weight in the stored layout (lay.cout, sum(lay.stored), 3, 3, 3), zero rows and
        columns for the pad channels; the weight itself when nothing is padded -- or a key of CONV_PACKS, built from that weight.  mode: the
        split-operand mode ("split", "poly"); c0: the stored width of the first source ("poly", "poly_wino", "w0"); device: take the device builder
        when the kind has one and the weight is on a GPU (arith.device_packs)."""
        if kind == "fp32" and lay is None:
            return self.packed()[0]
        cache, gen = param_cache(self, "_split_packs"), generation(self, lay)
        w = self.conv.weight if lay is None else cache.get(gen, "padded_weight", lambda: self._pad_weight(lay))
        if kind == "padded_weight":
            return w
        key, host, dev = CONV_PACKS[kind]
        key = key(mode, c0) if callable(key) else key
        if device and dev is not None and w.is_cuda:
            return cache.get(gen, ("device",) + (key if isinstance(key, tuple) else (key,)), lambda: dev(w, mode, c0))
        return cache.get(gen, key, lambda: host(w, mode, c0))

    def _pad_weight(self, lay):
        w = self.conv.weight.detach()
        wp = w.new_zeros((lay.cout, sum(lay.stored)) + tuple(w.shape[2:]))
        wp[:w.shape[0]] = to_stored(w.transpose(1, -1), lay.real, lay.stored).transpose(1, -1)
        return wp.contiguous()

    def _padded_weight(self, lay):
        return self.weight_pack("padded_weight", lay)

    def _norm_affine(self, ch, B, st0, st1, real=None, stored=None):
        """per-(sample, channel) affine of one normalisation layer from the statistics of what it normalises (real / stored: the channel
        layout of channel-padded sources, None: unpadded)"""
        if ch == "g":
            return ops.groupnorm_affine(st0, st1, self.groupnorm.num_groups, self.groupnorm.eps, self.groupnorm.weight.detach().float().contiguous(),
                                        self.groupnorm.bias.detach().float().contiguous(), real=real)
        bn = self.batchnorm                       # eval BatchNorm3d: running statistics
        sc = (bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps))
        sh = bn.bias.detach().double() - bn.running_mean.double() * sc
        if real is not None:                      # (zero scale and shift on the pads)
            sc, sh = to_stored(sc, real, stored), to_stored(sh, real, stored)
        return sc.float().expand(B, -1).contiguous(), sh.float().expand(B, -1).contiguous()

    def _run_generic(self, src0, src1, stats0, stats1, with_stats, lay=None):
        """every layer order but 'gcr' (see the class docstring)"""
        order, ic = self.order, self.order.index("c")
        B, cout = src0.shape[0], self.conv.out_channels if lay is None else lay.cout
        cin = src0.shape[-1] + (0 if src1 is None else src1.shape[-1])
        wp = self.weight_pack("fp32", lay)
        if ic == 0:
            a = torch.ones((B, cin), dtype=torch.float32, device=src0.device)
            d = torch.zeros_like(a)
        else:
            st0 = st1 = None
            if order[0] == "g":
                st0 = stats0 if stats0 is not None else ops.channel_stats(src0)
                st1 = None if src1 is None else (stats1 if stats1 is not None else ops.channel_stats(src1))
            a, d = self._norm_affine(order[0], B, st0, st1, *((None, None) if lay is None else (lay.real, lay.stored)))
        post = order[ic + 1:]
        bias = None if self.conv.bias is None else self.conv.bias.detach().float().contiguous()
        if bias is not None and lay is not None:
            bias = to_stored(bias, (self.conv.out_channels,), (cout,)).contiguous()
        out_lay = (None, None) if lay is None else ((self.conv.out_channels,), (cout,))
        fuse_relu = bias is None and post[:1] == "r"
        y = ops.conv3d_gcr(src0, src1, a, d, wp, cout, relu=fuse_relu)
        k = 1 if fuse_relu else 0
        if bias is not None:                      # conv bias, fused with the non-linearity that follows it (if one does)
            act = _ACT[post[0]][2] if post[:1] and post[0] in _ACT else ops.ACT_NONE
            ops.affine_act(y, bias=bias, act=act, out=y)
            k = 1 if act != ops.ACT_NONE else 0
        for ch in post[k:]:
            if ch in _ACT:
                ops.affine_act(y, act=_ACT[ch][2], out=y)
            else:
                na, nd = self._norm_affine(ch, B, ops.channel_stats(y) if ch == "g" else None, None, *out_lay)
                ops.affine_act(y, a=na, d=nd, out=y)
        return y, (ops.channel_stats(y) if with_stats else None)

    def run(self, src0, src1=None, stats0=None, stats1=None, with_stats=True, arith=None, rest0=None):
        """arith: the arith.Arith of this call (None: arith.DEFAULT).  src0 [B][D][H][W][C0] (full res), src1 [B][D/2][H/2][W/2][C1] or None -> ([B][D][H][W][Cout], output stats).
        stats0/stats1: (sum, sumsq, V) of the inputs when the producing kernel already emitted them.
        rest0 [B][C0]: (polyphase form of a decoder layer) the value the skip connection src0 holds away from the cells: its full-resolution
        launch takes the affine-in-weights form as well."""
        return self._run(src0, src1, stats0, stats1, with_stats, arith, None, rest0)[:2]

    def run_at_rest(self, src0, at_rest, stats0=None, with_stats=True, arith=None):
        """run() of a single-source layer behind gn_grid_scatter's volume -> (y, output stats, the AtRest of y or None).  at_rest: AtRest (None: run()).
        arith.sparse_first_conv: only the output tiles that can see an occupied cell (within at_rest.reach) go through the matrix cores; the rest
        are border-class constants taken from a dense launch of this layer over a small all-at-rest volume with the same affine: bit-identical output.
        arith.affine_in_weights (f16x2): the GroupNorm affine moves into per-sample weights and a bias table (ops.conv_affine_pack), so that
        the matrix cores multiply exact zeros wherever src0 is at rest -- same MACs, less power, more clock (csrc/conv_prep.hip).
        The AtRest handed back carries what this launch learned: its own output's rest value (affine-in-weights form) and its output over the small
        volume (occupancy-aware launch); None when it learned neither."""
        return self._run(src0, None, stats0, None, with_stats, arith, at_rest, None)

    def _run(self, src0, src1, stats0, stats1, with_stats, arith, at_rest, rest0):
        arith = arith or AR.DEFAULT
        lay = self._layout(src0, src1)
        if self.order != "gcr":
            return self._run_generic(src0, src1, stats0, stats1, with_stats, lay) + (None,)
        _, gamma, beta = self.packed()
        st0 = stats0 if stats0 is not None else ops.channel_stats(src0)
        st1 = None
        if src1 is not None:
            st1 = stats1 if stats1 is not None else ops.channel_stats(src1)
        cout = self.conv.out_channels if lay is None else lay.cout
        reach, value, small, flat = (0, None, None, None) if at_rest is None else (at_rest.reach, at_rest.value, at_rest.small, at_rest.flat)
        plan = conv_plan(arith, tuple(src0.shape[1:4]), src0.shape[-1], 0 if src1 is None else src1.shape[-1], cout, reach, value is not None,
                         None if small is None else tuple(small.shape[1:4]), flat is not None, rest0 is not None)
        if plan.mode == ops.CONV_FP32:
            a, d = ops.groupnorm_affine(st0, st1, self.groupnorm.num_groups, self.groupnorm.eps, gamma, beta, real=None if lay is None else lay.real)
            r, nxt = ops.conv3d_gcr(src0, src1, a, d, self.weight_pack("fp32", lay), cout, relu=True, with_stats=with_stats), None
        else:
            r, nxt = self._run_split(plan, src0, src1, st0, st1, with_stats, at_rest, gamma, beta, rest0, lay, device_packs=arith.device_packs)
        return (r + (nxt,)) if with_stats else (r, None, nxt)

    def _run_split(self, plan, src0, src1, st0, st1, with_stats, at_rest, gamma, beta, rest0, lay=None, device_packs=False):
        """execute a conv_plan on the split-operand kernels (16-bit matrix cores: csrc/unet_split.hip, unet_wino.hip, unet_wino32.hip) in one of two
        operand forms: literal (the GroupNorm affine applied while the halo is staged) or affine-in-weights (ops.conv_affine_pack) -> (the launch's
        result, the output's AtRest or None).
        lay: channel-padded storage (_Layout) -- the padded weight and stored widths in every pack, the GroupNorm over the real channels
        device_packs (arith.device_packs): the static packs come from the device builders (weight_pack); the launches are the same"""
        gn, weight, cout, mode, c0 = self.groupnorm, self.weight_pack("padded_weight", lay), self.conv.out_channels, plan.mode, src0.shape[-1]
        real = None
        if lay is not None:
            cout, real = lay.cout, lay.real

        def pack(kind):
            return self.weight_pack(kind, lay, mode=mode, c0=c0, device=device_packs)
        part = prep = act_inv = rest_out = None
        if plan.aiw and not plan.poly:
            # a layer whose input is at rest (0 for the scattered volume, at_rest.value behind it) almost everywhere
            a, d = ops.groupnorm_affine(st0, None, gn.num_groups, gn.eps, gamma, beta, real=real)
            prep = ops.conv_affine_pack(weight if weight.is_contiguous() else weight.contiguous(), a, d, st0, at_rest.value if at_rest.reach > 1 else None,
                                        wino=plan.wino)
            # away from the cells the operand is zero: the output is ReLU(0 * scale + K[interior]) = ReLU(K[63]) -- the next layer's rest value
            rest_out = torch.relu(prep.kbias[:, 63]).contiguous()
        else:
            # literal form.  fp16 planes: the sample's activations are range-normalised by a power of two (exact, undone in the epilogue)
            if mode == ops.SPLIT_F16X2:
                a, d, act_inv = ops.groupnorm_affine(st0, st1, gn.num_groups, gn.eps, gamma, beta, with_act_scale=True, real=real)
            else:
                a, d = ops.groupnorm_affine(st0, st1, gn.num_groups, gn.eps, gamma, beta, real=real)
            if plan.poly:
                pk0, pkm = pack("poly")
                part = ops.upconv_partial(src1, a[:, c0:].contiguous(), d[:, c0:].contiguous(), pkm, cout, act_inv=act_inv)
                if plan.aiw:
                    # the full-resolution part in the affine-in-weights form: the skip connection src0 is at rest away from the cells
                    # (a, d carry the sample's power-of-two activation scale: exact to undo)
                    a0 = (a[:, :c0] * act_inv[:, None]).contiguous()
                    d0 = (d[:, :c0] * act_inv[:, None]).contiguous()
                    prep = ops.conv_affine_pack(pack("w0"), a0, d0, st0, rest0, wino=plan.wino)
                else:
                    a, d = a[:, :c0].contiguous(), d[:, :c0].contiguous()
                    wpack = pack("poly_wino") if plan.wino else pk0
            else:
                wpack = pack("wino" if plan.wino else "split")
        # the one launch tail of each form (a polyphase launch reads the full-resolution source alone: the upsampled channels arrive as the partial)
        if prep is not None:
            launch = lambda x, **kw: ops.conv3d_gcr_split_persample(x, prep, relu=True, **kw)
        elif plan.wino:
            launch = lambda x, **kw: ops.conv3d_gcr_split_wino(x, a, d, wpack, cout, relu=True, act_inv=act_inv, **kw)
        else:
            launch = lambda x, **kw: ops.conv3d_gcr_split(x, None if plan.poly else src1, a, d, wpack, cout, relu=True, act_inv=act_inv, **kw)
        occ, small_out = {}, None
        if plan.small:
            # occupancy-aware: the border-class constants come from `launch` -- the kernel AND the pack the real launch takes -- over a small all-at-rest
            # volume (a plain dense launch); this layer's output there is the next layer's small volume
            B, n, reach = src0.shape[0], plan.small, at_rest.reach
            small_out = launch(at_rest.small if at_rest.small is not None else torch.zeros((B, n, n, n, c0), dtype=torch.float32, device=src0.device))
            occ = dict(tile_active=ops.grid_tile_flags(at_rest.flat, B, src0.shape[1:4], reach), kconst=_class_constants(small_out, reach, cout), kreach=reach)
        r = launch(src0, with_stats=with_stats, partial=part, **occ)
        learned = rest_out is not None or small_out is not None
        return r, (AtRest(at_rest.flat, at_rest.reach + 1, rest_out, small_out) if learned else None)


class DoubleConv(nn.Sequential):
    def __init__(self, in_channels, out_channels, encoder, kernel_size=3, order="gcr", num_groups=8):
        super().__init__()
        if encoder:
            c1_in, c1_out = in_channels, max(out_channels // 2, in_channels)
            c2_in, c2_out = c1_out, out_channels
        else:
            c1_in, c1_out = in_channels, out_channels
            c2_in, c2_out = out_channels, out_channels
        self.add_module("SingleConv1", SingleConv(c1_in, c1_out, kernel_size, order, num_groups))
        self.add_module("SingleConv2", SingleConv(c2_in, c2_out, kernel_size, order, num_groups))
        if encoder:              # (a decoder's first layer reads two sources: Decoder states their split)
            self.SingleConv1.in_real = (c1_in,)
        self.SingleConv2.in_real = (c2_in,)

    def run(self, src0, src1=None, stats0=None, stats1=None, sparse_flat=None, arith=None, rest0=None):
        """-> (y, stats, rest_out).  sparse_flat: src0 is gn_grid_scatter's volume (flat cell index of every scattered point): both convolutions run
        occupancy-aware / in the affine-in-weights form, and rest_out [B][Cout] is the value the block's output holds away from the cells (None when
        that form did not run); rest0: that value for src0 of a decoder block (its skip connection)"""
        if sparse_flat is None or src1 is not None:
            y, st = self.SingleConv1.run(src0, src1, stats0, stats1, arith=arith, rest0=rest0)
            return self.SingleConv2.run(y, None, st, arith=arith) + (None,)
        y, st, at_rest = self.SingleConv1.run_at_rest(src0, AtRest(sparse_flat, 1), stats0, arith=arith)
        y, st, at_rest = self.SingleConv2.run_at_rest(y, at_rest, st, arith=arith)
        return y, st, (None if at_rest is None else at_rest.value)


class Encoder(nn.Module):
    def __init__(self, in_channels, out_channels, apply_pooling=True, conv_layer_order="gcr", num_groups=8):
        super().__init__()
        self.pooling = nn.MaxPool3d(kernel_size=2) if apply_pooling else None
        self.basic_module = DoubleConv(in_channels, out_channels, encoder=True, order=conv_layer_order, num_groups=num_groups)

    def run(self, x, stats=None, sparse_flat=None, arith=None):
        """-> (y, stats, rest_out): DoubleConv.run's"""
        if self.pooling is not None:
            sparse_flat = None
            x, stats = ops.maxpool3d_2(x, with_stats=True)
        return self.basic_module.run(x, None, stats, sparse_flat=sparse_flat, arith=arith)


class Decoder(nn.Module):
    def __init__(self, in_channels, out_channels, conv_layer_order="gcr", num_groups=8):
        super().__init__()
        self.basic_module = DoubleConv(in_channels, out_channels, encoder=False, order=conv_layer_order, num_groups=num_groups)
        # cat((encoder_features [out_channels], x [in_channels - out_channels])): the split of Abstract3DUNet's decoders
        self.basic_module.SingleConv1.in_real = (out_channels, in_channels - out_channels)

    def run(self, encoder_features, x, stats_skip=None, stats_x=None, arith=None, skip_rest=None):
        # cat((encoder_features, upsample_nearest(x)), dim=channel) is never materialised
        return self.basic_module.run(encoder_features, x, stats_skip, stats_x, arith=arith, rest0=skip_rest)[:2]


class FinalConv1x1(PackedModule, nn.Conv3d):
    in_stored = None         # the stored width of its channel-padded input (Abstract3DUNet); None: in_channels

    def stored_weight(self):
        """the weight as (out_channels, stored input channels): zero columns for the pad channels of the input"""
        w = self.weight.detach().reshape(self.out_channels, self.in_channels)
        return to_stored(w, (self.in_channels,), (self.in_stored or self.in_channels,))

    def _pack(self):
        return pack_wb(self.stored_weight(), self.bias)

    def run(self, x):
        wp, b, k = self.packed()
        shp = x.shape
        if shp[-1] != k:
            raise ValueError(f"FinalConv1x1: input of {shp[-1]} channels, expected {k}")
        y = ops.linear(x.reshape(-1, shp[-1]), wp, b, None, None, relu=False, K=k)
        return y.reshape(*shp[:-1], self.out_channels)


class Abstract3DUNet(nn.Module):
    def __init__(self, in_channels, out_channels, final_sigmoid=False, basic_module=DoubleConv, f_maps=64, layer_order="gcr",
                 num_groups=8, num_levels=4, is_segmentation=False, testing=False, **kwargs):
        super().__init__()
        if basic_module is not DoubleConv or is_segmentation:
            raise NotImplementedError("only the DoubleConv regression UNet of the GarmentNets pipeline is implemented")
        if isinstance(f_maps, int):
            f_maps = number_of_features_per_level(f_maps, num_levels=num_levels)
        self.f_maps = list(f_maps)
        self.encoders = nn.ModuleList([
            Encoder(in_channels if i == 0 else f_maps[i - 1], f, apply_pooling=i > 0, conv_layer_order=layer_order, num_groups=num_groups)
            for i, f in enumerate(f_maps)])
        rf = list(reversed(f_maps))
        self.decoders = nn.ModuleList([
            Decoder(rf[i] + rf[i + 1], rf[i + 1], conv_layer_order=layer_order, num_groups=num_groups) for i in range(len(rf) - 1)])
        self.final_conv = FinalConv1x1(f_maps[0], out_channels, 1)
        self.final_conv.in_stored = stored_channels(f_maps[0])
        self.final_activation = None
        self.in_channels = in_channels
        self.arith = None        # arithmetic of forward(x) (None: arith.DEFAULT); run() takes it per call

    def check_input(self, x):
        """refuse, by name, the shapes this UNet does not run: NotImplementedError"""
        if x.shape[-1] % 16 != 0:
            raise NotImplementedError(f"Abstract3DUNet.run: an input stored with {x.shape[-1]} channels is not a multiple of 16 (the first convolution "
                                      "reads 16 channels at a time): hand it channel-padded (stored_channels), as forward() and the volume aggregator do")
        k = 2 ** (len(self.encoders) - 1)
        if any(int(n) % k != 0 for n in x.shape[1:4]):
            raise NotImplementedError(f"Abstract3DUNet: grid {tuple(x.shape[1:4])} does not halve evenly through {len(self.encoders)} levels "
                                      f"(every dimension must be a multiple of {k}: only x2 nearest upsampling is implemented)")

    def run(self, x, stats=None, pre_final=False, return_stats=False, sparse_flat=None, arith=None):
        """channel-last in, channel-last out (pre_final: stop before the final 1x1x1 convolution -- it is linear, so the decoders can
        fold it into their first layer and sample the f_maps[0]-channel volume instead: networks/conv_implicit_wnf.py UNetResult).  Every kernel that produces a tensor also emits the per-channel statistics the
        next GroupNorm needs (conv / max-pool epilogues), so no activation is re-read for normalisation.
        Widths that are not multiples of 32 run channel-padded (stored_channels): the pre-final volume then holds stored_channels(f_maps[0])
        channels, the pads exactly zero; the final convolution's output has out_channels."""
        self.check_input(x)
        feats = []
        for i, enc in enumerate(self.encoders):
            x, stats, rest_out = enc.run(x, stats, sparse_flat=sparse_flat if i == 0 else None, arith=arith)
            feats.insert(0, (x, stats, rest_out))      # rest_out: encoder 0 behind a scattered volume (affine-in-weights form)
        for dec, (skip, skip_stats, skip_rest) in zip(self.decoders, feats[1:]):
            x, stats = dec.run(skip, x, skip_stats, stats, arith=arith, skip_rest=skip_rest)
        if pre_final:       # return_stats: + (sum, sumsq, V) of the pre-final volume (the decoders derive their input scale from it)
            return (x, stats) if return_stats else x
        return self.final_conv.run(x)

    def forward(self, x):
        """x: (B, C, D, H, W) as in the reference; returns (B, C', D, H, W) (a view over channel-last storage)."""
        return self.run(*stored_input(x), arith=self.arith).permute(0, 4, 1, 2, 3)


def stored_input(x):
    """(B,C,D,H,W) -> (the stored volume run() reads, its statistics or None): stored_volume(x) with the producer's statistics (_gn_stats); an input
    width the first convolution does not read as it is goes channel-padded, pads 0, and without them"""
    stats = getattr(x, "_gn_stats", None)
    v = stored_volume(x)
    if v.shape[-1] % 16 != 0:
        v, stats = to_stored(v, (v.shape[-1],), (stored_channels(v.shape[-1]),)), None
    return v, stats


def stored_volume(x):
    """(B,C,D,H,W) -> the channel-last storage the UNet reads: the channel-padded volume a scattered (B,C,D,H,W) view carries
    (VolumeFeatureAggregator, C not a multiple of 16), else to_channel_last(x)"""
    v = getattr(x, "_gn_stored", None)
    return to_channel_last(x) if v is None else v


def to_channel_last(x):
    """(B,C,D,H,W) tensor (any strides) -> contiguous [B][D][H][W][C]; free when x already is a channel-last view."""
    return x.permute(0, 2, 3, 4, 1).contiguous()
