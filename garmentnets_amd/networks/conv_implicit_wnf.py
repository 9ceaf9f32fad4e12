"""ConvImplicitWNFPipeline (inference) -- API twin of /root/reference/networks/conv_implicit_wnf.py:23-338.

Keeps the reference's class names, constructor kwargs, sub-module names (= checkpoint schema: ``pointnet2_nocs``,
``volume_agg.local_nn``, ``unet_3d.abstract_3d_unet``, ``volume_decoder.mlp`` ...), stage methods
(``pointnet2_forward``, ``unet3d_forward``, ``volume_decoder_forward``, ``surface_decoder_forward``,
``mc_surface_decoder_forward``, ``forward``) and result-dict keys, so that predict.py is a drop-in.  ``validation_metrics`` gives the
losses of the reference's infer (:405-452); ``training_step`` / ``training_metrics`` / ``configure_optimizers`` are the second stage's training step (garmentnets_amd/train_pipeline.py, imported on use: the loss gradients of gn_value_losses_bwd and optim.FusedAdam, as the first stage's train.py); ``vis_batch`` renders the reference's monitor images on the device (garmentnets_amd.visualize).  Feature volumes are stored channel-last; the (B,C,D,H,W) tensors handed out are views.
"""
import functools
import os
import threading
import weakref
from typing import Callable, NamedTuple, Optional

import torch
from torch import nn

from .. import arith as AR
from .. import ops
from ..batch import Batch
from ..components.mlp import MLP, PackedModule, fold_batchnorm, generation, param_cache
from ..components.unet3d import Abstract3DUNet, DoubleConv, stored_channels, stored_volume, to_channel_last
from ..components.pointnet2 import Segments
from .pointnet2_nocs import PointNet2NOCS


def agg_stored_channels(c):
    """the stored width of the scattered volume with c real channels: c when the first convolution reads it as it is (a multiple of 16), else
    rounded up as the UNet stores its activations (components/unet3d.py stored_channels), the pads exact zeros"""
    return int(c) if int(c) % 16 == 0 else stored_channels(c)


class VolumeFeatureAggregator(nn.Module):
    """per-point MLP -> scatter (any torch_scatter reduction: max | mean | sum | add | min | mul) into a (B,C,G,G,G) volume -- conv_implicit_wnf.py:23-100.
    Empty cells hold what torch_scatter 2.0.8 leaves there: 0, and 1 under 'mul'."""

    def __init__(self, nn_channels=[1024, 1024, 128], batch_norm=True, lower_corner=(0, 0, 0), upper_corner=(1, 1, 1),
                 grid_shape=(32, 32, 32), reduce_method="mean", include_point_feature=True, include_confidence_feature=False):
        super().__init__()
        self.local_nn = MLP(nn_channels, batch_norm=batch_norm)
        self.lower_corner = tuple(lower_corner)
        self.upper_corner = tuple(upper_corner)
        self.grid_shape = tuple(grid_shape)
        if reduce_method not in ops.REDUCE_CODES:
            raise ValueError(f"VolumeFeatureAggregator: reduce_method={reduce_method!r} is not a torch_scatter reduction ({sorted(ops.REDUCE_CODES)})")
        self.reduce_method = reduce_method
        self.include_point_feature = include_point_feature
        self.include_confidence_feature = include_confidence_feature

    def prefetch_zero(self, B, device):
        """zero-fill the (B, G, G, G, C) volume of the NEXT forward() on a side stream, now: the fill (17 GB at batch 16, 128^3: 3 ms of
        pure HBM writes) then runs next to PointNet++'s serial farthest-point sampling (16 workgroups on 256 CUs) instead of after it.
        Only callers that WILL run forward() next ask for it (ConvImplicitWNFPipeline.forward, predict._dense_phase) and they call
        drop_prefetch() on their way out, so the buffer never outlives the step that asked for it."""
        if not PREFETCH_ZERO or not torch.cuda.is_available() or torch.cuda.is_current_stream_capturing():
            return
        C = self.local_nn[-1][0].out_features if self.local_nn is not None else None
        if C is None:
            return
        C = agg_stored_channels(C)
        dev = _normalise_device(device)
        state = _THREAD_STATE.of(self)
        pre = state.get("prezero")
        if pre is not None and pre[0] == B and pre[1].device == dev:
            return                                   # an earlier prefetch of this shape was never consumed: still zero
        if B * int(torch.tensor(self.grid_shape).prod()) * C * 4 < (64 << 20):
            return                                   # small volumes: the in-stream memset costs microseconds
        main = torch.cuda.current_stream(dev)
        side = state.get("side")
        if side is None or side.device != dev:
            side = state["side"] = torch.cuda.Stream(device=dev)
        side.wait_stream(main)                       # the blocks the allocator hands out were last used on the main stream
        with torch.cuda.stream(side):
            vol, cnt = ops.zeroed_volume(B, self.grid_shape, C, dev)
            ev = torch.cuda.Event()
            ev.record(side)
        state["prezero"] = (B, vol, cnt, ev)

    def drop_prefetch(self):
        """release an unconsumed prefetch_zero buffer (17 GB at batch 16, 128^3)"""
        pre = _THREAD_STATE.of(self).pop("prezero", None)
        if pre is not None:
            pre[1].record_stream(torch.cuda.current_stream(pre[1].device))     # filled on the side stream, freed from this one

    def forward(self, nocs_data):
        B = nocs_data.num_graphs
        conf = nocs_data.pred_confidence
        feats, flat = ops.grid_features(nocs_data.x, nocs_data.pos.contiguous(), nocs_data.sim_points.float().contiguous(),
                                        conf.contiguous(), nocs_data.batch, self.lower_corner, self.upper_corner, self.grid_shape,
                                        self.include_point_feature, self.include_confidence_feature)
        if self.local_nn is not None:
            feats = self.local_nn(feats)
        C = feats.shape[1]
        Cs = agg_stored_channels(C)
        if Cs != C:                                   # channel-padded rows: zeros on the pads, which every reduction keeps at zero
            padded = torch.zeros((feats.shape[0], Cs), dtype=torch.float32, device=feats.device)
            padded[:, :C] = feats
            feats = padded
        pre = _THREAD_STATE.of(self).pop("prezero", None)
        prezeroed = None
        if pre is not None and torch.cuda.is_current_stream_capturing():
            pre = None                                # a captured graph must own its memset: never bake "already zero" into it
        if pre is not None and pre[0] == B and pre[1].shape[-1] == feats.shape[1] and pre[1].device == feats.device:
            cur = torch.cuda.current_stream(feats.device)
            cur.wait_event(pre[3])
            pre[1].record_stream(cur)                 # filled on the side stream, consumed (and outlived) by work on this one: the allocator
            pre[2].record_stream(cur)                 # must not hand the block to the side stream's NEXT fill while that work is in flight
            prezeroed = (pre[1], pre[2])
        if self.reduce_method == "mul":
            # a 'mul' volume is 1 wherever no point landed: no statistics from the occupied cells alone and no occupancy-aware convolution behind it
            # (both assume empty cells are 0) -- the UNet takes the dense launch with whole-volume statistics
            vol = ops.grid_scatter(feats, flat, B, self.grid_shape, "mul", prezeroed=prezeroed, c_real=C)
            stats = flat = None
        else:
            vol, stats = ops.grid_scatter(feats, flat, B, self.grid_shape, self.reduce_method, with_stats=True, prezeroed=prezeroed, c_real=C)   # [B][G][G][G][Cs]
        out = vol.permute(0, 4, 1, 2, 3) if Cs == C else vol[..., :C].permute(0, 4, 1, 2, 3)
        if Cs != C:
            out._gn_stored = vol   # the channel-padded storage: the UNet reads it without a copy
        if stats is not None:
            out._gn_stats = stats  # GroupNorm statistics of the (mostly empty) volume, from its occupied cells only
            out._gn_flat = flat    # the occupied cells: the first UNet convolution only visits the tiles that can see one
        return out


class _PerThreadState:
    """per (host thread, module instance) scratch state: the prefetched zero volume and its side stream belong to the thread that asked
    for them -- two threads sharing one model never consume or drop each other's buffer (no shared mutable state on the
    call path).  Entries die with the module (weak keys) or the thread."""

    def __init__(self):
        self._tls = threading.local()

    def of(self, module):
        table = self._tls.__dict__.setdefault("table", weakref.WeakKeyDictionary())
        st = table.get(module)
        if st is None:
            st = table[module] = {}
        return st


_THREAD_STATE = _PerThreadState()


def _normalise_device(device):
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class UNet3D(nn.Module):
    def __init__(self, in_channels, out_channels, f_maps=64, layer_order="gcr", num_groups=8, num_levels=4):
        super().__init__()
        self.abstract_3d_unet = Abstract3DUNet(in_channels=in_channels, out_channels=out_channels, final_sigmoid=False,
                                               basic_module=DoubleConv, f_maps=f_maps, layer_order=layer_order,
                                               num_groups=num_groups, num_levels=num_levels, is_segmentation=False)

    def forward(self, data):
        return self.abstract_3d_unet(data)


class DecoderPack(NamedTuple):
    """the kernel-side parameters of one ImplicitWNFDecoder on rows of c0 channels"""
    fp32: tuple                                  # three (w, b, sc, sh, n) layers as ops.implicit_decode takes them (csrc/decode.hip)
    split: Optional[ops.DecodeSplitPack]         # the same layers for the 16-bit matrix cores (csrc/decode_split.hip), or None
    c0: int

    def facts(self):
        """what decode_plan reads of it: (has a split-operand pack, c0, hidden width, out_channels)"""
        return self.split is not None, self.c0, self.fp32[0][4], self.fp32[2][4]


class DecodeSource(NamedTuple):
    """what a decoder samples from: the UNet's pre-final volume with the folded pack (ImplicitWNFDecoder.run_on) or the decoder's own input volume"""
    vol: torch.Tensor                            # (B, D, H, W, C) channel-last
    pack: Optional[DecoderPack]
    scales: Callable                             # smax -> (B, 4) per-garment input scales of the split-operand kernels (ops.decoder_input_scale)


LATTICE, BATCHED, SPLIT, FUSED, MLP_LAYERS = "lattice", "batched", "split", "fused", "mlp"


class DecodePlan(NamedTuple):
    """which launches one decoder call takes (decode_plan)"""
    path: str        # LATTICE | BATCHED | SPLIT | FUSED | MLP_LAYERS
    chunk: int       # rows per sampler launch of the chunked paths (SPLIT, FUSED, MLP_LAYERS)
    scales: bool     # a split-operand kernel runs: it takes the garment's input scale, and the gated fp32 twin follows it when there is one


@functools.lru_cache(maxsize=1024)      # (pure, of hashable arguments; bounded: M is whatever a caller queries)
def decode_plan(arith, fused, pack, dims, contiguous, Q, B, M, chunk_rows, batch_bytes, out_packed):
    """The launches of one decoder call from the arithmetic, the module's `fused` switch, DecoderPack.facts() (None: no fused kernel takes the decoder),
    the volume's (D, H, W) and contiguity, the lattice edge Q (None: B x M query points), the row budget of a chunk, the byte budget of the batched
    launches, and whether the output's row sets lie back to back.  No tensor, no library entry.
      MLP_LAYERS  no fused kernel (only [C0, N1, N2, out <= 4] with N1, N2 multiples of 256 has one), or `fused` off: sampler, gn_linear per layer
      FUSED       sampler, gn_implicit_decode: the three layers in one fp32 kernel, hidden activations stay in LDS
      SPLIT       (the shipped widths under Arith.decode_mode "f16x2") sampler, split-operand decoder on the 16-bit matrix cores
      BATCHED     SPLIT for the queries of a whole batch in one set of launches, while the sampled rows fit the cache they are handed over in
      LATTICE     lattice queries of the folded scalar decoder (Arith.fused_lattice) in ONE launch per garment: the kernel walks bricks of 4 x 8 x 8
                  lattice points out of LDS, no sampled-row buffer; the lattice must be at least as fine as the volume (ops.lattice_split_shapes)
    The first three go garment by garment, a separate high-occupancy sampler feeding the MLP through a buffer of `chunk` rows.  Behind every
    split-operand launch its fp32 twin follows, gated on the device by the garment's `unsafe` flag."""
    if Q is not None:                               # lattice: whole i-slabs per chunk (the brick sampler's unit)
        chunk_rows = max(1, chunk_rows // (Q * Q)) * Q * Q
    if not fused or pack is None:
        return DecodePlan(MLP_LAYERS, chunk_rows, False)
    split, c0, hidden, out_channels = pack
    if not (split and arith.decode_mode == "f16x2"):
        return DecodePlan(FUSED, chunk_rows, False)
    if Q is not None:
        brick = arith.fused_lattice and contiguous and ops.lattice_split_shapes(dims, c0, hidden, out_channels, Q)
        return DecodePlan(LATTICE if brick else SPLIT, chunk_rows, True)
    batched = B >= 2 and M > 0 and contiguous and out_packed and B * M * ops.pad4(c0) * 4 <= batch_bytes
    return DecodePlan(BATCHED if batched else SPLIT, chunk_rows, True)


class ImplicitWNFDecoder(PackedModule):
    """trilinear feature sampling (border, align_corners) -> MLP -- conv_implicit_wnf.py:120-149.

    forward, decode_lattice and run_on each name a DecodeSource and _run executes the DecodePlan that decode_plan (which describes the paths) gives
    for it.  run_on folds the UNet's final 1x1x1 convolution into the first layer (folded_pack) and samples the pre-final volume; when it cannot
    (Arith.fold_final_conv off, a decoder no fused kernel takes) it decodes the materialised volume like forward."""

    # 2^20 rows x 32 channels = 134 MB: half a 128^3 lattice, stays in the 256 MB Infinity Cache (2^18 rows: 1 ms slower per step; the whole lattice: no faster)
    ROWS_PER_CHUNK = int(os.environ.get("GARMENTNETS_DECODE_CHUNK", 1 << 20))
    # the surface decoders of predict.py:184-187 fit (16 x ~49 000 vertices x 32 channels = 100 MB); larger query sets go garment by garment
    BATCH_ROWS_BYTES = int(os.environ.get("GARMENTNETS_DECODE_BATCH_BYTES", 192 << 20))
    fused = True

    def __init__(self, nn_channels=(128, 512, 512, 1), batch_norm=True):
        super().__init__()
        self.mlp = MLP(list(nn_channels), batch_norm=batch_norm)
        self.nn_channels = tuple(nn_channels)
        self.out_channels = nn_channels[-1]
        self.arith = None          # arithmetic of a direct call (None: arith.DEFAULT); the pipeline passes its own per call

    def _fusable(self, c0):
        ch = self.nn_channels
        return len(ch) == 4 and c0 % 32 == 0 and ch[1] % 256 == 0 and ch[2] % 256 == 0 and ch[3] <= 4

    def _build_pack(self, c0, split_shapes, fold=None):
        """-> DecoderPack on rows of c0 channels; fold: (Wf, bf) in fp64, a linear map in front of the first layer (W1' = W1 Wf, b1' = b1 + W1 bf); split_shapes:
        the (c0, hidden) that also get the split-operand pack (csrc/decode_split.hip): the shipped 256 on either input, the class default 512 folded"""
        ch = self.nn_channels
        layers, raw = [], []
        for i, block in enumerate(self.mlp):
            w, b = block[0].weight.detach(), block[0].bias.detach()
            if i == 0 and fold is not None:
                b = b.double() + w.double() @ fold[1]
                w = w.double() @ fold[0]
            w, b = w.float(), b.float().contiguous()
            sc, sh = fold_batchnorm(block[2]) if len(block) > 2 else (None, None)
            layers.append((ops.pack_kpair(w) if i < 2 else w.contiguous(), b, sc, sh, ch[i + 1]))
            raw.append((w, b, sc, sh))
        split = ops.pack_decode_split(raw).to(w.device) if ch[1] == ch[2] and (c0, ch[1]) in split_shapes else None
        return DecoderPack(tuple(layers), split, c0)

    def _pack(self):
        return self._build_pack(self.nn_channels[0], ((128, 256),)) if self._fusable(self.nn_channels[0]) else None

    def folded_pack(self, final_conv):
        """The same decoder with the UNet's final 1x1x1 convolution (linear, no activation) folded into its first layer (fp64 on the host).  It runs on rows
        sampled from the PRE-final feature volume (f_maps[0] = 32 channels instead of 128): trilinear interpolation is linear and its weights sum to one, so
        sample(Wf x + bf) = Wf sample(x) + bf up to rounding.  The 128-channel volume is then never written or read (17 GB per 16-garment batch at 128^3), the
        sampler moves a quarter of the bytes and layer 1 does a quarter of the FLOPs.  -> DecoderPack, or None when not foldable.  A channel-padded pre-final
        volume (f_maps[0] not a multiple of 32: components/unet3d.py stored_channels) gets zero weight columns for its pad channels."""
        cin = final_conv.in_stored or final_conv.in_channels
        if not (self.fused and self._fusable(cin) and self.nn_channels[0] == final_conv.out_channels and final_conv.kernel_size == (1, 1, 1)):
            return None
        # (both modules' parameters AND buffers: _build_pack folds the BatchNorm running statistics in)
        return param_cache(self, "_folded").get(generation(self, id(final_conv), cin, generation(final_conv)), "folded", lambda: self._build_pack(
            cin, ((32, 256), (32, 512)), (final_conv.stored_weight().double(), final_conv.bias.detach().double())))

    def _plan(self, arith, vol, pack, Q, M, out_packed=True):
        """decode_plan for a (B, D, H, W, C) channel-last volume: Q rows per lattice edge, or (Q None) M query points per garment"""
        contiguous = (vol if Q is None else vol[:1]).is_contiguous()       # the batched launches read the batch, the lattice kernel one garment
        return decode_plan(arith, self.fused, None if pack is None else pack.facts(), tuple(vol.shape[1:4]), contiguous, Q, vol.shape[0], M,
                           self.ROWS_PER_CHUNK, self.BATCH_ROWS_BYTES, out_packed)

    def _decode_rows(self, plan, vol_b, out, pack, query=None, Q=0, xscale=None):
        """one garment of a LATTICE, SPLIT, FUSED or MLP_LAYERS plan.  vol_b [D][H][W][C]; out [M][OUT]; query [M][3], or None: the (Q,Q,Q) lattice;
        xscale: the garment's (s, 1/s, unsafe, 0) row of ops.decoder_input_scale"""
        M = out.shape[0]
        if plan.path == LATTICE:
            ops.implicit_decode_lattice_split(vol_b, Q, pack.split, out, xscale=xscale)
            if xscale is not None:          # garments the device marked unsafe for fp16 planes: the gated fp32 twin samples for itself
                ops.implicit_decode(vol_b, pack.fp32, Q=Q, m0=0, M=M, out=out, run_if=xscale[2:3])
            return
        buf = ops.new_rows(min(M, plan.chunk), vol_b.shape[-1], vol_b.device)
        for m0 in range(0, M, plan.chunk):
            m = min(plan.chunk, M - m0)
            if query is not None:
                s = ops.trilinear_sample(vol_b, query=query[m0:m0 + m], out=buf[:m])
            else:
                s = ops.trilinear_sample(vol_b, Q=Q, m0=m0, M=m, out=buf[:m])
            if plan.path == SPLIT:
                ops.implicit_decode_split(s, pack.split, out=out[m0:m0 + m], xscale=xscale)
                if xscale is not None:      # the garments the device marked unsafe for fp16 planes: gated fp32 twin (a no-op otherwise)
                    ops.implicit_decode(None, pack.fp32, M=m, out=out[m0:m0 + m], xin=s, run_if=xscale[2:3])
            elif plan.path == FUSED:
                ops.implicit_decode(None, pack.fp32, M=m, out=out[m0:m0 + m], xin=s)
            else:
                out[m0:m0 + m] = self.mlp(s)

    def _run(self, src, query_points, Q, arith):
        """query_points (B,M,3) -> (B,M,out); query_points None -> the (Q,Q,Q) lattice -> (B,Q,Q,Q[,out])"""
        vol, pack, scales = src
        q = None if query_points is None else query_points.float().contiguous()
        B, Q, M = (vol.shape[0], Q, Q * Q * Q) if q is None else (vol.shape[0], None, q.shape[1])
        out = torch.empty((B, M, self.out_channels), dtype=torch.float32, device=vol.device)
        plan = self._plan(arith, vol, pack, Q, M, out.stride(0) == M * out.stride(1))
        xs = scales(pack.split.smax) if plan.scales else None
        if plan.path == BATCHED:            # three launches for the whole batch: sampler, decoder, gated fp32 twin -- row for row what the garment loop gives
            rows = ops.trilinear_sample_batch(vol, q)
            ops.implicit_decode_split_batch(rows, pack.split, out, xscale=xs)
            ops.implicit_decode_batch(rows, pack.fp32, out, run_if=xs[:, 2:], run_if_stride=xs.stride(0))
        else:
            for b in range(B):
                self._decode_rows(plan, vol[b], out[b], pack, None if q is None else q[b], Q, None if xs is None else xs[b])
        return out if q is not None else out.reshape(B, Q, Q, Q, self.out_channels).squeeze(-1)

    def _tensor_source(self, features_grid):
        """the decoder's own (B,C,D,H,W) input.  Its scales take one gn_channel_stats pass, remembered ON the caller's tensor object with its version counter
        (the reference's chunk loop calls the decoder 8 times per garment on one volume): the entry dies with the tensor, never mistaken for a recycled one"""
        vol = to_channel_last(features_grid)

        def scales(smax):
            cached = getattr(features_grid, "_gn_chan_stats", None)
            if cached is None or cached[0] != features_grid._version:
                cached = (features_grid._version, ops.channel_stats(vol))
                try:
                    features_grid._gn_chan_stats = cached
                except AttributeError:
                    pass
            return ops.decoder_input_scale(cached[1][1], cached[1][2], smax)
        return DecodeSource(vol, self.packed(), scales)

    def forward(self, features_grid, query_points, arith=None):
        """features_grid (B,C,D,H,W), query_points (B,M,3) in [0,1] -> (B,M,out)"""
        return self._run(self._tensor_source(features_grid), query_points, None, arith or self.arith or AR.DEFAULT)

    def decode_lattice(self, features_grid, Q, arith=None):
        """All (Q,Q,Q) lattice queries of predict.py:145-157 without materialising them -> (B,Q,Q,Q[,out])"""
        return self._run(self._tensor_source(features_grid), None, Q, arith or self.arith or AR.DEFAULT)

    def run_on(self, unet3d_result, query_points=None, Q=0, arith=None):
        """decode against a unet3d_forward result: on its pre-final volume (UNetResult) when this decoder can absorb the final convolution, else on the
        materialised 128-channel volume.  query_points (B,M,3) -> (B,M,out); query_points None -> the (Q,Q,Q) lattice -> (B,Q,Q,Q[,out])"""
        arith = arith or self.arith or AR.DEFAULT
        pack = self.folded_pack(unet3d_result.final_conv) if isinstance(unet3d_result, UNetResult) and arith.fold_final_conv else None
        if pack is None:
            return self._run(self._tensor_source(unet3d_result["out_feature_volume"]), query_points, Q, arith)
        return self._run(DecodeSource(unet3d_result.pre_final, pack, unet3d_result.input_scales), query_points, Q, arith)


# zero-fill of the scattered volume overlapped with PointNet++ (VolumeFeatureAggregator.prefetch_zero)
PREFETCH_ZERO = os.environ.get("GARMENTNETS_PREFETCH_ZERO", "1") != "0"

class UNetResult(dict):
    """unet3d_forward's result: {'out_feature_volume': (B,128,D,H,W)} as in the reference, except that the 128-channel volume is
    only materialised (one gn_linear over all voxels) if somebody actually reads it; the decoders do not (see folded_pack)."""

    def __init__(self, pre_final, final_conv, pre_stats=None):
        super().__init__()
        self.pre_final, self.final_conv = pre_final, final_conv          # [B][D][H][W][f_maps[0]] channel-last (channel-padded: pads 0)
        self.pre_stats = pre_stats                                       # (sum, sumsq, V) of pre_final from the last conv's epilogue, or None
        self._scales = {}                                                # smax -> (B, 2) decoder input scales

    def input_scales(self, smax):
        """(B, 2) run-time input scales (s, 1/s) of the split-operand decoder kernel for this volume (ops.decoder_input_scale)"""
        if smax not in self._scales:
            if self.pre_stats is None:
                self.pre_stats = ops.channel_stats(self.pre_final)
            self._scales[smax] = ops.decoder_input_scale(self.pre_stats[1], self.pre_stats[2], smax)
        return self._scales[smax]

    def select(self, b0, b1):
        """the same result for garments b0..b1-1 (predict.py slices out_feature_volume[[i]] per sample)"""
        st = None if self.pre_stats is None else (self.pre_stats[0][b0:b1], self.pre_stats[1][b0:b1], self.pre_stats[2])
        sub = UNetResult(self.pre_final[b0:b1], self.final_conv, st)
        sub._scales = {k: v[b0:b1] for k, v in self._scales.items()}
        if dict.__contains__(self, "out_feature_volume"):
            dict.__setitem__(sub, "out_feature_volume", dict.__getitem__(self, "out_feature_volume")[b0:b1])
        return sub

    def _materialise(self):
        if not dict.__contains__(self, "out_feature_volume"):
            dict.__setitem__(self, "out_feature_volume", self.final_conv.run(self.pre_final).permute(0, 4, 1, 2, 3))

    def __getitem__(self, k):
        if k == "out_feature_volume":
            self._materialise()
        return dict.__getitem__(self, k)

    def __contains__(self, k):
        return k == "out_feature_volume" or dict.__contains__(self, k)

    def keys(self):
        self._materialise()
        return dict.keys(self)

    def items(self):
        self._materialise()
        return dict.items(self)

    def get(self, k, default=None):
        return self[k] if k in self else default

    # the rest of the Mapping surface sees the reference's one-key dict too (CPython's dict(u3) / copy / len fast paths bypass keys())
    def values(self):
        self._materialise()
        return dict.values(self)

    def __iter__(self):
        self._materialise()
        return dict.__iter__(self)

    def __len__(self):
        return 1

    def copy(self):
        self._materialise()
        return dict(dict.items(self))

    def __reduce__(self):
        self._materialise()
        return (dict, (dict(dict.items(self)),))

    def __repr__(self):
        return "UNetResult(out_feature_volume=%s)" % ("<lazy>" if not dict.__contains__(self, "out_feature_volume") else tuple(dict.__getitem__(self, "out_feature_volume").shape),)


class ConvImplicitWNFPipeline(nn.Module):
    def __init__(self, pointnet2_params, volume_agg_params, unet3d_params, volume_decoder_params, surface_decoder_params,
                 mc_surface_decoder_params=None, learning_rate=1e-4, loss_type="l2", volume_loss_weight=1.0,
                 surface_loss_weight=1.0, mc_surface_loss_weight=0, volume_classification=False, volume_task_space=False,
                 vis_per_items=0, max_vis_per_epoch_train=0, max_vis_per_epoch_val=0, batch_size=None):
        super().__init__()
        self.hparams = dict(pointnet2_params=dict(pointnet2_params), volume_agg_params=dict(volume_agg_params),
                            unet3d_params=dict(unet3d_params), volume_decoder_params=dict(volume_decoder_params),
                            surface_decoder_params=dict(surface_decoder_params),
                            mc_surface_decoder_params=None if mc_surface_decoder_params is None else dict(mc_surface_decoder_params),
                            mc_surface_loss_weight=mc_surface_loss_weight, volume_task_space=volume_task_space,
                            learning_rate=learning_rate, loss_type=loss_type, volume_loss_weight=volume_loss_weight,
                            surface_loss_weight=surface_loss_weight, volume_classification=volume_classification, vis_per_items=vis_per_items,
                            max_vis_per_epoch_train=max_vis_per_epoch_train, max_vis_per_epoch_val=max_vis_per_epoch_val)
        self.pointnet2_nocs = PointNet2NOCS(**pointnet2_params)
        self.volume_agg = VolumeFeatureAggregator(**volume_agg_params)
        self.unet_3d = UNet3D(**unet3d_params)
        self.volume_decoder = ImplicitWNFDecoder(**volume_decoder_params)
        self.surface_decoder = ImplicitWNFDecoder(**surface_decoder_params)
        self.mc_surface_decoder = None
        if mc_surface_loss_weight > 0:
            self.mc_surface_decoder = ImplicitWNFDecoder(**mc_surface_decoder_params)
        self.volume_task_space = volume_task_space
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.loss_type = loss_type
        self.volume_loss_weight = volume_loss_weight
        self.surface_loss_weight = surface_loss_weight
        self.mc_surface_loss_weight = mc_surface_loss_weight
        self.volume_classification = volume_classification
        self.vis_per_items = vis_per_items
        self.max_vis_per_epoch_train = max_vis_per_epoch_train
        self.max_vis_per_epoch_val = max_vis_per_epoch_val
        self.arith = AR.DEFAULT      # this model's arithmetic (an immutable arith.Arith); every stage method also takes arith= per call

    # -- checkpoint ------------------------------------------------------------------------------------------
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location="cpu", **overrides):
        """Reads a Lightning-style checkpoint {'state_dict', 'hyper_parameters'} (predict.py:101) without Lightning."""
        ckpt = torch.load(checkpoint_path, map_location=map_location, weights_only=False)
        hp = dict(ckpt["hyper_parameters"])
        hp.update(overrides)
        model = cls(**hp)
        model.load_state_dict(ckpt["state_dict"])
        return model

    def save_checkpoint(self, path):
        torch.save({"state_dict": self.state_dict(), "hyper_parameters": self.hparams}, path)

    @property
    def device(self):
        return self.pointnet2_nocs.device

    # -- stages ----------------------------------------------------------------------------------------------
    def pointnet2_forward(self, data, prefetch_volume=False):
        """prefetch_volume: the caller runs unet3d_forward next (and volume_agg.drop_prefetch() on its way out): start the zero-fill
        of the feature volume beside PointNet++ (VolumeFeatureAggregator.prefetch_zero)"""
        sizes = data._sizes if hasattr(data, "_sizes") else None
        if prefetch_volume and sizes is not None and data.pos.is_cuda:   # (no host sizes: the batch size would cost a device synchronisation here)
            self.volume_agg.prefetch_zero(len(sizes), data.pos.device)
        seg = Segments.of(data.batch, sizes if sizes is not None else getattr(data, "sizes", None))     # the batch's sizes travel with THIS call
        result = self.pointnet2_nocs(data, seg=seg)
        bins = self.pointnet2_nocs.nocs_bins
        _, confidence, pred_nocs = ops.nocs_head(result["per_point_logits"], bins)
        result["nocs_data"] = Batch(sizes=seg.sizes, x=result["per_point_features"], pos=pred_nocs, batch=result["per_point_batch_idx"],
                                    sim_points=data.pos, pred_confidence=confidence)
        return result

    def unet3d_forward(self, pointnet2_result, arith=None):
        arith = arith or self.arith
        in_feature_volume = self.volume_agg(pointnet2_result["nocs_data"])
        net = self.unet_3d.abstract_3d_unet
        pre, st = net.run(stored_volume(in_feature_volume), getattr(in_feature_volume, "_gn_stats", None), pre_final=True, return_stats=True,
                          sparse_flat=getattr(in_feature_volume, "_gn_flat", None), arith=arith)
        return UNetResult(pre, net.final_conv, st)   # ['out_feature_volume'] materialises the reference's tensor on demand

    def volume_decoder_forward(self, unet3d_result, query_points, arith=None):
        out = self.volume_decoder.run_on(unet3d_result, query_points, arith=arith or self.arith)
        return {"out_features": out, "pred_volume_value": out.view(*out.shape[:-1])}

    def surface_decoder_forward(self, unet3d_result, query_points, arith=None):
        return {"out_features": self.surface_decoder.run_on(unet3d_result, query_points, arith=arith or self.arith)}

    def mc_surface_decoder_forward(self, unet3d_result, query_points, arith=None):
        return {"out_features": self.mc_surface_decoder.run_on(unet3d_result, query_points, arith=arith or self.arith)}

    def volume_lattice_forward(self, unet3d_result, volume_size, arith=None):
        """Whole (Q,Q,Q) WNF volume per garment in one pass (replaces the 64^3 chunk loop of predict.py:145-157)."""
        return {"pred_volume": self.volume_decoder.run_on(unet3d_result, None, Q=volume_size, arith=arith or self.arith)}

    @staticmethod
    def get_aabb_scale_offset(aabb, padding=0.05):
        """conv_implicit_wnf.py:299-313: per-sample scale / offset that maps the task-space bounding box (B,2,3) into the unit NOCS cube
        (x, y centred on 0.5, the top of z at 1 - padding)"""
        nocs_radius = 0.5 - padding
        radius = torch.max(torch.abs(aabb), dim=1)[0][:, :2]
        radius_scale = torch.min(nocs_radius / radius, dim=1)[0]
        z_scale = (nocs_radius * 2) / (aabb[:, 1, 2] - aabb[:, 0, 2])
        scale = torch.minimum(radius_scale, z_scale)
        offset = torch.full((len(aabb), 3), 0.5, dtype=aabb.dtype, device=aabb.device)
        offset[:, 2] = 1 - padding - aabb[:, 1, 2] * scale
        return scale, offset

    def apply_volume_task_space(self, data, pointnet2_result):
        """conv_implicit_wnf.py:279-297: the gridding runs on the normalised SIMULATION coordinates of the points instead of their
        predicted NOCS coordinates (first sample's scale / offset for the whole batch, as the reference)"""
        scale, offset = self.get_aabb_scale_offset(data.cloth_sim_aabb.to(data.pos.device))
        nd = pointnet2_result["nocs_data"]
        new_nd = Batch(sizes=nd._sizes, **{k: getattr(nd, k) for k in nd.keys})
        new_nd.pos = ((data.pos * scale[0]) + offset[0]).to(torch.float32).contiguous()
        out = dict(pointnet2_result)
        out["nocs_data"] = new_nd
        return out

    def forward(self, data, arith=None):
        """conv_implicit_wnf.py:315-338"""
        arith = arith or self.arith
        try:
            p2 = self.pointnet2_forward(data, prefetch_volume=True)
            if self.volume_task_space:
                p2 = self.apply_volume_task_space(data, p2)
            u3 = self.unet3d_forward(p2, arith)
        finally:
            self.volume_agg.drop_prefetch()
        result = {
            "pointnet2_result": p2,
            "unet3d_result": u3,
            "volume_decoder_result": self.volume_decoder_forward(u3, data.volume_query_points, arith),
            "surface_decoder_result": self.surface_decoder_forward(u3, data.surf_query_points, arith),
        }
        if self.mc_surface_decoder is not None:
            result["mc_surface_decoder_result"] = self.mc_surface_decoder_forward(u3, data.mc_surf_query_points, arith)
        return result

    # -- validation ------------------------------------------------------------------------------------------
    LOSS_TYPES = ("l2", "smooth_l1")

    def validation_metrics(self, data, arith=None, result=None):
        """the loss dict of the reference's infer (conv_implicit_wnf.py:405-452) as python floats: volume_loss, surface_loss[, mc_surface_loss
        when mc_surface_loss_weight > 0] (each its weight times the mean criterion) and loss, their sum.  data: the network input plus the
        targets io.dataset draws (volume_query_points / gt_volume_value, surf_query_points / gt_sim_points[, mc_surf_query_points /
        is_query_point_on_surf]).  Criterion: loss_type (l2 = MSE, smooth_l1 with beta 1); the volume takes BCE-with-logits when
        volume_classification, the mc surface always.  forward() runs the decoders, ONE gn_value_losses launch the three losses.  result: this
        model's forward(data) when the caller already has it."""
        self._check_loss_type()
        return self.losses_from(self.forward(data, arith) if result is None else result, data)

    def _check_loss_type(self):
        if self.loss_type not in self.LOSS_TYPES:
            raise ValueError(f"Invalid loss_type: {self.loss_type!r} (expected one of {self.LOSS_TYPES})")

    def loss_segments(self, result, data):
        """-> (segments, names, weights) of the weighted loss of infer, in its order: the volume (BCE-with-logits when volume_classification, else
        loss_type), the surface (loss_type) and, when mc_surface_loss_weight > 0, the mc surface (BCE-with-logits).  segments are (pred, target, kind)
        as ops.value_losses and the differentiable value_loss take them: validation (losses_from) and the training step (train_pipeline.loss_and_sums) read
        this one list"""
        self._check_loss_type()
        segs = [(result["volume_decoder_result"]["pred_volume_value"], data.gt_volume_value, "bce_logits" if self.volume_classification else self.loss_type),
                (result["surface_decoder_result"]["out_features"], data.gt_sim_points, self.loss_type)]
        names, weights = ["volume_loss", "surface_loss"], [self.volume_loss_weight, self.surface_loss_weight]
        if self.mc_surface_loss_weight > 0:
            segs.append((result["mc_surface_decoder_result"]["out_features"], data.is_query_point_on_surf, "bce_logits"))
            names.append("mc_surface_loss")
            weights.append(self.mc_surface_loss_weight)
        return segs, names, weights

    @staticmethod
    def metrics_from_sums(sums, names, weights, counts):
        """the loss dict from the per-segment sums (python floats) of the loss kernel: each weight times the mean criterion, and loss, their sum"""
        metrics = {k: w * (s / n) for k, w, s, n in zip(names, weights, sums, counts)}
        metrics["loss"] = sum(metrics.values())
        return metrics

    def losses_from(self, result, data):
        """validation_metrics' loss dict from a forward() result dict and the batch's targets"""
        segs, names, weights = self.loss_segments(result, data)
        sums = ops.value_losses(segs)[:, 0].cpu().tolist()
        return self.metrics_from_sums(sums, names, weights, [seg[1].numel() for seg in segs])

    # -- monitors (garmentnets_amd/visualize.py) ---------------------------------------------------------------
    def vis_batch(self, batch, batch_idx, result, is_train=False, img_size=256, backend="device"):
        """the reference's vis_batch (conv_implicit_wnf.py:345-403) -> {label: (2 S, 2 S, 4) fp32 image}, labels train_<vis_idx> / val_<vis_idx>: per
        selected garment (get_vis_idxs over vis_per_items / max_vis_per_epoch_* / batch_size) the NOCS pair of the first stage with the
        ground-truth and the predicted grip point, above the pair of WNF slices (0.5 < y < 0.6 of the volume queries: target and prediction, the
        sigmoid of the logits when volume_classification).  result: this model's forward of the batch; all images of the batch in one launch
        pair.  No garment selected: nothing is launched, nothing synchronises."""
        from .. import visualize as V
        picked = V.monitor_selection(self, batch_idx, batch.nocs_grip_point.shape[0], is_train)
        if not picked:
            return {}
        with torch.no_grad():
            pred_nocs = result["pointnet2_result"]["nocs_data"].pos
            pred_value = result["volume_decoder_result"]["pred_volume_value"].detach()
            if self.volume_classification:
                pred_value = torch.sigmoid(pred_value)
            rows = V.garment_rows(batch)
            specs = []
            for i, _ in picked:
                pred = rows(pred_nocs, i)
                specs += V.nocs_pair_specs(rows(batch.y, i), pred, batch.nocs_grip_point[i], V.grip_row(rows(batch.pos, i), pred))
                specs += V.wnf_pair_specs(batch.volume_query_points[i], batch.gt_volume_value[i], pred_value[i])
            images = V.render_batch(specs, img_size, backend)
        return dict(zip([label for _, label in picked], V.compose(images, 4)))

    # -- training (garmentnets_amd/train_pipeline.py; imported on use: the inference modules do not depend on the training code) ----------------------
    def training_step(self, batch, batch_idx=None):
        """the reference's loss of one batch: a device scalar with a graph through every parameter of the second stage (the first stage is frozen)"""
        from .. import train_pipeline
        return train_pipeline.training_step(self, batch, batch_idx)

    def training_metrics(self, batch):
        """validation_metrics' keys for the model AS IT STANDS (training-mode BatchNorm included), detached python floats, from the sums of the
        loss kernel: one forward"""
        from .. import train_pipeline
        return train_pipeline.training_metrics(self, batch)

    def configure_optimizers(self):
        """the reference's optim.Adam(self.parameters(), lr=self.learning_rate): the frozen first stage's parameters are in the group, never get
        a gradient, and FusedAdam skips them"""
        from ..optim import FusedAdam
        return FusedAdam(self.parameters(), lr=self.learning_rate, modules=self)
