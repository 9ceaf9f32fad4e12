"""Differentiable bindings of the point and grid operators, under the third-party call shapes INTEGRATION.md section B documents, and of the 3-D UNet.

The reference's dense layers (nn.Linear, BatchNorm1d, Conv3d, GroupNorm, ...) have torch's own backward on ROCm.  The third-party operators
between them (torch_cluster.fps / radius, PointConv's gather + max, global_max_pool, knn_interpolate, torch_scatter.scatter, F.grid_sample) are
the ones this package restates in HIP; here each gets a ``torch.autograd.Function`` whose forward is the existing op, unchanged, and whose backward
is a kernel of csrc/grad.hip.  A reference-side module that binds these functions can take gradients on an MI355X.

The UNet is not a torch graph (channel-last, channel-padded volumes, GroupNorm folded into the conv's operand load, concat and upsampling never
materialised), so it gets its own backward: ``conv3d_gcr`` / ``max_pool3d_2`` / ``unet3d`` run the existing forward kernels and differentiate them with
csrc/unet_grad.hip (DESIGN.md "UNet gradients"); its final 1x1x1 convolution is a linear block of the next paragraph.  With
``arith.Arith.conv_grad_mode = "f16x2"`` the two gradients of every 3x3x3 convolution run on the 16-bit matrix cores instead (csrc/unet_grad_split.hip,
``unet3d.conv_grad_plan``; DESIGN.md "f16x2 backward of the UNet convolutions"); the default is the fp32 backward, launch for launch.

The dense layers of this package (components.mlp.MLPStack, HipLinear) hold torch parameters but evaluate through ``gn_linear``, which torch's autograd
cannot see: ``mlp`` / ``linear`` run the same forward kernels block by block, keep each block's input and ReLU output, and differentiate them with
csrc/linear_grad.hip (DESIGN.md "MLP gradients"); ``implicit_decode`` is the decoder as the chain ``grid_sample_points`` -> ``mlp``.  With these a
gradient flows from a torch loss on the decoder's prediction to every parameter of the second stage, and into PointNet++ through
``point_conv_max(local_nn=lambda e: mlp(stack, e))``.

``mlp(..., batch_stats=True)`` gives a BatchNorm in training mode torch's semantics: the batch's own mean and biased variance over all rows, the
gradient through both, the running buffers updated in place (DESIGN.md "Train-mode BatchNorm").

``nocs_bin_loss`` / ``value_loss`` close the chain: the forward is the validation kernels of csrc/losses.hip, unchanged (the loss value is
``validation_metrics``' to the last bit), the backward their gradient kernels, which take the mirror decision on the device from the forward's own
sums.  The optimiser is optim.FusedAdam, the first stage's training step train.py (DESIGN.md "Training step, first stage"), the second stage's
train_pipeline.py (DESIGN.md "Training step, second stage": ``mlp`` -> ``scatter`` -> ``unet3d`` -> ``implicit_decode`` per head -> ``value_loss``).

What this is NOT: a backward for the fused inference kernels (the fused / split-operand decoder,
``gn_sa_fused``: ``implicit_decode`` and ``point_conv_max`` are the unfused chains).  The inference modules do not import this file.

Selections (max / min) hand the gradient to ONE element per (slot, channel): among equal values the lowest point / edge index (torch_scatter's CUDA
choice is whichever thread wins an atomic: parity unpinned).  Every sum is ordered: identical calls give identical bits.
"""
import torch

import torch.nn.functional as F

from . import arith as AR
from . import ops
from .components import unet3d as U
from .components.mlp import HipLinear, MLPStack, fold_batchnorm, generation, pack_linear, pack_wb, param_cache
from .components.pointnet2 import Segments, _example_self_src

__all__ = ["fps", "radius", "ball_table", "point_conv_max", "global_max_pool", "knn_interpolate", "scatter", "grid_sample_points",
           "conv3d_gcr", "max_pool3d_2", "unet3d", "mlp", "linear", "implicit_decode", "nocs_bin_loss", "value_loss"]


# ------------------------------------------------------------------------------------------------ index results (no gradient)
def fps(pos, batch, ratio=0.5, random_start=False):
    """torch_cluster.fps(pos, batch, ratio): int64 indices of the sampled points.  random_start=False (the first point of each example) is this
    package's pinned choice; an index result, not differentiable."""
    seg = Segments.of(batch)
    with torch.no_grad():
        cseg = Segments([ops.fps_count(n, ratio) for n in seg.sizes], pos.device)
        start = None
        if random_start:
            start = torch.tensor([int(torch.randint(0, max(n, 1), (1,))) for n in seg.sizes], dtype=torch.int32).to(pos.device)
        idx = ops.fps(pos.detach().contiguous(), seg.ptr, cseg.ptr, max(seg.sizes) if seg.sizes else 0, cseg.total, start)
    return idx.long()


def ball_table(x, y_idx, r, batch_x, batch_y, max_num_neighbors=32):
    """The radius graph as gn_ball_query's table: (nbr int32 [M][K] -- the first K points within r of centre x[y_idx[c]], ascending index, -1 padded --
    and cnt int32 [M]).  ``point_conv_max`` takes this form."""
    seg, cseg = Segments.of(batch_x), Segments.of(batch_y)
    with torch.no_grad():
        return ops.ball_query(x.detach().contiguous(), seg.ptr, y_idx.to(torch.int32), cseg.ptr, r, int(max_num_neighbors))


def radius(x, y_idx, r, batch_x, batch_y, max_num_neighbors=32):
    """torch_cluster.radius(x, x[y_idx], r, batch_x, batch_y, max_num_neighbors) -> edge_index (2, E) int64: row = centre, col = point of x."""
    nbr, _ = ball_table(x, y_idx, r, batch_x, batch_y, max_num_neighbors)
    row, col = (nbr >= 0).nonzero(as_tuple=True)
    return torch.stack((row, nbr[row, col].long()))


# ------------------------------------------------------------------------------------------------ PointConv(local_nn, aggr='max')
class _SaGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos, centre_idx, nbr, self_loops, self_src):
        edges, slot_src, _ = ops.sa_gather(x, pos, centre_idx, nbr, self_loops=self_loops, self_src=self_src)
        ctx.save_for_backward(slot_src)
        ctx.x_shape = tuple(x.shape)
        ctx.mark_non_differentiable(slot_src)
        return edges, slot_src

    @staticmethod
    def backward(ctx, grad_edges, _):
        (slot_src,) = ctx.saved_tensors
        n, c = ctx.x_shape
        gx = ops.sa_gather_bwd(grad_edges, slot_src, c, n) if ctx.needs_input_grad[0] else None
        return gx, None, None, None, None, None


class _SegmentMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, slot_src, M, S):
        out = ops.segment_max(h, slot_src, M, S)
        ctx.save_for_backward(h, out, slot_src)
        ctx.ms = (M, S)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, out, slot_src = ctx.saved_tensors
        return ops.segment_max_bwd(grad_out, out, h, slot_src, *ctx.ms), None, None, None


def point_conv_max(x, pos, centre_idx, nbr, local_nn, add_self_loops=True, self_loop_scope="batch", batch=None, batch_centre=None, real_edges=False):
    """PointConv(local_nn, aggr='max') over the radius graph ``nbr`` (``ball_table``): edge rows [x_j, pos_j - pos_i] -> ``local_nn`` (any
    nn.Module, torch's own backward) -> max per centre.  Differentiable in x and in local_nn's parameters; positions are data.  The unfused chain
    gn_sa_gather + local_nn + gn_segment_max.  self_loop_scope="example" (needs batch / batch_centre): the self-loop rule per example, as
    components.pointnet2.SAModule applies it.  real_edges=True: ``local_nn`` sees the rows of real edges only (PyG's edge set: the empty slots of the
    table are indexed out with torch and the result copied back into a zero buffer, whose empty rows gn_segment_max never reads), so a training
    BatchNorm inside it takes its statistics over exactly PyG's rows."""
    centre_idx = centre_idx.to(torch.int32)
    M, K = nbr.shape
    S = K + (1 if add_self_loops else 0)
    self_src = None
    if add_self_loops and self_loop_scope == "example":
        seg, cseg = Segments.of(batch), Segments.of(batch_centre)
        if seg.num > 1:
            self_src = _example_self_src(seg.sizes, cseg.sizes, pos.device)
    pos = pos.detach().contiguous()
    if x is None:
        edges, slot_src, _ = ops.sa_gather(None, pos, centre_idx, nbr, self_loops=add_self_loops, self_src=self_src)
    else:
        edges, slot_src = _SaGather.apply(ops.fp32_rows(x, "x"), pos, centre_idx, nbr, add_self_loops, self_src)
    if real_edges and local_nn is not None:
        rows = (slot_src >= 0).nonzero().squeeze(1)
        hc = local_nn(edges.index_select(0, rows))
        h = hc.new_zeros((M * S, hc.shape[1])).index_copy(0, rows, hc)
    else:
        h = local_nn(edges) if local_nn is not None else edges
    return _SegmentMax.apply(ops.fp32_rows(h, "local_nn(edges)"), slot_src, M, S)


# ------------------------------------------------------------------------------------------------ global_max_pool
class _GlobalMaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, ptr, B):
        out = ops.global_max_pool(h, ptr, B)
        ctx.save_for_backward(h, out, ptr)
        ctx.B = B
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, out, ptr = ctx.saved_tensors
        return ops.global_max_pool_bwd(grad_out, out, h, ptr, ctx.B), None, None


def global_max_pool(x, batch):
    """torch_geometric.nn.global_max_pool(x, batch) -> (B, C)"""
    seg = Segments.of(batch)
    return _GlobalMaxPool.apply(ops.fp32_rows(x, "x"), seg.ptr, seg.num)


# ------------------------------------------------------------------------------------------------ knn_interpolate
class _KnnInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos_x, ptr_x, pos_y, ptr_y, k):
        out = ops.knn_interpolate(x, pos_x, ptr_x, pos_y, ptr_y, k)
        ctx.save_for_backward(pos_x, ptr_x, pos_y, ptr_y)
        ctx.k, ctx.n = k, x.shape[0]
        return out

    @staticmethod
    def backward(ctx, grad_y):
        pos_x, ptr_x, pos_y, ptr_y = ctx.saved_tensors
        # the forward keeps no index tensor: the same search again (ascending (d2, index), the forward kernels' order)
        nbr, d2 = ops.knn_neighbours(pos_x, ptr_x, pos_y, ptr_y, ctx.k)
        return ops.knn_interpolate_bwd(grad_y, nbr, d2, ctx.n), None, None, None, None, None


def knn_interpolate(x, pos_x, pos_y, batch_x, batch_y, k=3):
    """torch_geometric.nn.knn_interpolate(x, pos_x, pos_y, batch_x, batch_y, k): gradient to the features x only -- the neighbour search and the
    weights sit under no_grad in torch_geometric too."""
    seg_x, seg_y = Segments.of(batch_x), Segments.of(batch_y)
    return _KnnInterpolate.apply(ops.fp32_rows(x, "x"), pos_x.detach().contiguous(), seg_x.ptr, pos_y.detach().contiguous(), seg_y.ptr, int(k))


# ------------------------------------------------------------------------------------------------ torch_scatter.scatter
class _GridScatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, flat_idx, cells, reduce):
        vol = ops.grid_scatter(rows, flat_idx, 1, (cells,), reduce).view(cells, rows.shape[1])
        if reduce in ("max", "min"):
            ctx.save_for_backward(flat_idx, vol, rows)       # the winner test reads the stored output and the input
        else:
            ctx.save_for_backward(flat_idx)                  # mean: the cell counts are counted again from flat_idx (one int32 per cell)
        ctx.reduce, ctx.n = reduce, rows.shape[0]
        return vol

    @staticmethod
    def backward(ctx, grad_vol):
        flat_idx, *rest = ctx.saved_tensors
        vol, rows = rest if rest else (None, None)
        return ops.grid_scatter_bwd(grad_vol.contiguous(), flat_idx, ctx.n, ctx.reduce, vol=vol, src=rows), None, None, None


def scatter(src, index, dim=-1, dim_size=None, reduce="mean"):
    """torch_scatter.scatter(src (C, N), index (N,), dim=-1, dim_size, reduce) -> (C, dim_size), the call of networks/conv_implicit_wnf.py:92-94.
    Empty cells hold 0 (1 under 'mul').  'mul' runs forward-only: asking for its gradient is a ValueError."""
    if reduce not in ops.REDUCE_CODES:
        raise ValueError(f"scatter: reduce={reduce!r} is not one of {sorted(ops.REDUCE_CODES)}")
    if src.dim() != 2 or dim not in (-1, 1) or index.dim() != 1 or index.numel() != src.shape[1]:
        raise ValueError("scatter: this binding takes src (C, N), index (N,) and dim=-1")
    if dim_size is None:
        dim_size = int(index.max().item()) + 1 if index.numel() else 0
    if reduce == "mul" and torch.is_grad_enabled() and src.requires_grad:
        raise ValueError("scatter: reduce='mul' has no gradient here (nobody trains with it; it divides by zero at a zero factor)")
    rows = ops.fp32_rows(src.t(), "src")
    return _GridScatter.apply(rows, index.to(torch.int32).contiguous(), int(dim_size), reduce).t()


# ------------------------------------------------------------------------------------------------ F.grid_sample
class _TrilinearSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vol, query):
        out = ops.trilinear_sample_batch(vol, query)
        ctx.save_for_backward(vol, query)
        return out

    @staticmethod
    def backward(ctx, grad_rows):
        vol, query = ctx.saved_tensors
        return ops.trilinear_sample_bwd(grad_rows, vol, query, want_vol=ctx.needs_input_grad[0], want_query=ctx.needs_input_grad[1])


def grid_sample_points(volume, query):
    """ImplicitWNFDecoder.forward's sampling: F.grid_sample(volume (N, C, D, H, W), 2 * query - 1, mode='bilinear', padding_mode='border',
    align_corners=True) at query (N, M, 3) in [0, 1] -> features (N, M, C).  Differentiable in the volume and in the query (a coordinate clamped
    at the border gets gradient 0, F.grid_sample's rule).  The volume gradient is an ordered sum per voxel: no float atomics."""
    if volume.dim() != 5 or query.dim() != 3 or query.shape[0] != volume.shape[0] or query.shape[2] != 3:
        raise ValueError("grid_sample_points: volume must be (N, C, D, H, W) and query (N, M, 3)")
    if volume.dtype != torch.float32 or query.dtype != torch.float32:
        raise TypeError("grid_sample_points: volume and query must be torch.float32")
    return _TrilinearSample.apply(volume.permute(0, 2, 3, 4, 1).contiguous(), query.contiguous())


# ------------------------------------------------------------------------------------------------ the 3-D UNet
def _tensor_stats(st):
    """(sum, sumsq, V) -> the two tensors an autograd.Function can take / return, and V"""
    return (None, None, 0) if st is None else (st[0], st[1], int(st[2]))


class _ConvGcr(torch.autograd.Function):
    """one 'gcr' SingleConv on stored volumes.  weight / gamma / beta are the module's own parameters (the forward is SingleConv.run on the module's
    packs of them); they are saved, so the backward differentiates the parameters the forward used and an in-place update in between is an autograd
    version error, not a silent gradient of the new values.  Returns (y, sum, sumsq): the output and its statistics (the next layer's GroupNorm)."""

    @staticmethod
    def forward(ctx, src0, src1, weight, gamma, beta, s0, q0, s1, q1, conv, arith):
        st0 = (s0, q0, src0[0].numel() // src0.shape[-1])
        st1 = None if src1 is None else (s1, q1, src1[0].numel() // src1.shape[-1])
        y, st = conv.run(src0, src1, st0, st1, arith=arith)
        ctx.save_for_backward(src0, src1, y, s0, q0, s1, q1, weight, gamma, beta)
        ctx.conv = conv
        ctx.arith = arith
        ctx.mark_non_differentiable(st[0], st[1])
        return y, st[0], st[1]

    @staticmethod
    def backward(ctx, grad_y, _gs, _gq):
        """One body for every unet3d.conv_grad_plan.  Under ("fp32", "fp32") -- the default -- the launches are those of csrc/unet_grad.hip alone.  With a
        gradient on the split-operand kernels (arith.conv_grad_mode = "f16x2") one masking pass (gn_relu_mask_max) serves both: the masked gradient g,
        its per-sample maximum and the power-of-two scales from it, found on the device.  The weight gradient then reads the forward's operand with the
        sample's activation scale (the affine of the f16x2 forward); the data gradient is the forward's direct split kernel on the pack of the flipped /
        transposed weight.  The GroupNorm backward stays fp32."""
        src0, src1, y, s0, q0, s1, q1, weight, gamma, beta = ctx.saved_tensors
        conv, gn, arith = ctx.conv, ctx.conv.groupnorm, ctx.arith or AR.DEFAULT
        need = ctx.needs_input_grad
        lay = conv._layout(src0, src1)
        S0, S1 = src0.shape[-1], 0 if src1 is None else src1.shape[-1]
        plan = U.conv_grad_plan(arith, tuple(src0.shape[1:4]), S0, S1, y.shape[-1])
        real = None if lay is None else lay.real
        st0 = (s0, q0, src0[0].numel() // S0)
        st1 = None if src1 is None else (s1, q1, src1[0].numel() // S1)
        gamma = gamma.detach().float().contiguous()
        dy = grad_y.contiguous()
        need_data = any(need[i] for i in (0, 1, 3, 4))
        g = gmax = scale = inv = None
        if (need[2] and plan.weight == "f16x2") or (need_data and plan.data == "f16x2"):
            g, gmax, scale, inv = ops.relu_mask_max(y, dy)
        dw = None
        if need[2]:
            beta = beta.detach().float().contiguous()
            if plan.weight == "f16x2":
                a, d, x_inv = ops.groupnorm_affine(st0, st1, gn.num_groups, gn.eps, gamma, beta, with_act_scale=True, real=real)
                dw = ops.conv3d_bwd_weight_split(src0, src1, a, d, None, g, x_inv=x_inv, gmax=gmax)      # (g is masked already: no second read of y)
            else:
                a, d = ops.groupnorm_affine(st0, st1, gn.num_groups, gn.eps, gamma, beta, real=real)
                dw = ops.conv3d_bwd_weight(src0, src1, a, d, y, dy)
            if lay is not None:                   # stored -> real channels (the pad rows / columns are exact zeros)
                cols = torch.cat([torch.arange(r, device=dw.device) + o for r, o in zip(lay.real, (0, S0))])
                dw = dw[:conv.conv.out_channels].index_select(1, cols)
        if not need_data:
            return None, None, dw, None, None, None, None, None, None, None, None
        # d operand = conv_transpose(g, W): the forward kernels on the flipped / transposed pack.  (The saved weight IS conv.conv.weight at the forward's
        # version -- unpacking it has checked that -- so the module's generation-keyed cache holds its packs.)
        cin_p = -(-(S0 + S1) // 32) * 32
        if plan.data == "f16x2":
            dxn = ops.conv3d_bwd_data_split(g, scale, inv, conv.weight_pack("bwd_data_split", lay, device=arith.device_packs), cin_p)
        else:
            dxn = ops.conv3d_bwd_data(g if g is not None else ops.relu_mask(y, dy), conv.weight_pack("bwd_data", lay), cin_p)
        t0 = ops.groupnorm_bwd_stats(dxn, 0, src0)
        t1 = None if src1 is None else ops.groupnorm_bwd_stats(dxn, S0, src1, half=True)
        p, q, r, dgamma, dbeta = ops.groupnorm_bwd_coef(t0, t1, st0, st1, gn.num_groups, gn.eps, gamma, real=real)
        d0 = ops.groupnorm_bwd_apply(dxn, 0, src0, p, q, r, 0) if need[0] else None
        d1 = ops.groupnorm_bwd_apply(dxn, S0, src1, p, q, r, S0, half=True) if src1 is not None and need[1] else None
        return d0, d1, dw, dgamma if need[3] else None, dbeta if need[4] else None, None, None, None, None, None, None


def _check_gcr(conv):
    if not isinstance(conv, U.SingleConv):
        raise TypeError(f"expected a components.unet3d.SingleConv, got {type(conv).__name__}")
    if conv.order != "gcr":
        raise NotImplementedError(f"layer order {conv.order!r} has no gradient here: only 'gcr' (GroupNorm -> Conv3d -> ReLU) is differentiable")


def _conv(conv, src0, src1, st0, st1, arith):
    """-> (y, (sum, sumsq, V) of y).  st0 / st1: the inputs' statistics when their producer emitted them (else one gn_channel_stats pass)"""
    if st0 is None:
        st0 = ops.channel_stats(src0.detach())
    if src1 is not None and st1 is None:
        st1 = ops.channel_stats(src1.detach())
    s1, q1, _ = _tensor_stats(st1)
    gn = conv.groupnorm
    y, s, q = _ConvGcr.apply(src0, src1, conv.conv.weight, gn.weight, gn.bias, st0[0], st0[1], s1, q1, conv, arith)
    return y, (s, q, y[0].numel() // y.shape[-1])


def _stored(t, name):
    if t.dim() != 5 or t.dtype != torch.float32:
        raise ValueError(f"{name}: expected a float32 channel-last stored volume [B][D][H][W][C], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def conv3d_gcr(single_conv, src0, src1=None, arith=None):
    """One 'gcr' ``SingleConv`` (GroupNorm -> Conv3d 3x3x3 -> ReLU) as a differentiable function of src0, src1 and the module's conv.weight,
    groupnorm.weight, groupnorm.bias.  src0 [B][D][H][W][C0] and the optional half-resolution src1 [B][D/2][H/2][W/2][C1] are channel-last STORED
    volumes (channel-padded when the module's in_real says so); the result is the stored output [B][D][H][W][stored Cout].  Forward: SingleConv.run
    (the kernels ``arith`` selects, dense launch).  Backward: csrc/unet_grad.hip -- an fp32 backward whatever the forward arithmetic, unless
    ``arith.conv_grad_mode`` is "f16x2": then the layer's two convolution gradients take the kernels unet3d.conv_grad_plan names (csrc/unet_grad_split.hip)."""
    _check_gcr(single_conv)
    return _conv(single_conv, _stored(src0, "src0"), None if src1 is None else _stored(src1, "src1"), None, None, arith)[0]


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, with_stats):
        ctx.save_for_backward(x)
        if with_stats:
            out, (s, q, _) = ops.maxpool3d_2(x, with_stats=True)
        else:
            out = ops.maxpool3d_2(x)
            s = q = x.new_empty(0, dtype=torch.float64)
        ctx.mark_non_differentiable(s, q)
        return out, s, q

    @staticmethod
    def backward(ctx, grad_out, _gs, _gq):
        (x,) = ctx.saved_tensors
        return ops.maxpool3d_2_bwd(grad_out.contiguous(), x), None


def _pool(x):
    """-> (pooled, its statistics): Encoder.run's call of ops.maxpool3d_2"""
    out, s, q = _MaxPool.apply(x, True)
    return out, (s, q, out[0].numel() // x.shape[-1])


def max_pool3d_2(x):
    """nn.MaxPool3d(2) on a channel-last stored volume [B][D][H][W][C] (even D, H, W; C % 4 == 0).  The gradient goes to the first maximum of each
    window in (z, y, x) order, a NaN winning (ATen's CPU scan); the winner is found again from the stored input, no index tensor is kept."""
    x = _stored(x, "x")
    if any(n % 2 for n in x.shape[1:4]):
        raise ValueError(f"max_pool3d_2: the volume {tuple(x.shape[1:4])} must have even dimensions")
    return _MaxPool.apply(x, False)[0]


def _unet_layers(model):
    return [sc for blk in list(model.encoders) + list(model.decoders) for sc in (blk.basic_module.SingleConv1, blk.basic_module.SingleConv2)]


def unet3d(model, x, arith=None):
    """``Abstract3DUNet.forward``'s contract -- x (B, C, D, H, W) -> (B, C', D, H, W), a view over channel-last storage -- differentiable in x and in
    every parameter of the model: ``conv3d_gcr`` per layer, ``max_pool3d_2`` between the encoder levels, the final 1x1x1 convolution as a row GEMM.
    Any f_maps / num_levels the forward runs; on channel-padded widths the pad gradients are exact zeros and reach no parameter.  arith: the
    arithmetic of the FORWARD kernels (None: model.arith, else arith.DEFAULT); the backward is fp32 throughout unless arith.conv_grad_mode is "f16x2"
    (the 3x3x3 convolutions' gradients on the 16-bit matrix cores, unet3d.conv_grad_plan; GroupNorm, max-pool and the final convolution stay fp32).  Layer orders other than 'gcr' raise
    NotImplementedError.  Under torch.no_grad(), or when nothing requires a gradient, this is model.forward's launches and nothing is saved."""
    if not isinstance(model, U.Abstract3DUNet):
        raise TypeError(f"unet3d: expected a components.unet3d.Abstract3DUNet, got {type(model).__name__}")
    for sc in _unet_layers(model):
        _check_gcr(sc)
    arith = arith if arith is not None else model.arith
    if not _needs_grad(model, x):
        with torch.no_grad():
            return model.run(*U.stored_input(x), arith=arith).permute(0, 4, 1, 2, 3)
    if x.dim() != 5 or x.dtype != torch.float32:
        raise ValueError(f"unet3d: expected a float32 (B, C, D, H, W) volume, got {x.dtype} {tuple(x.shape)}")
    # model.forward's reading of its input: an x that needs no gradient may carry its channel-padded storage and the producer's statistics
    # (VolumeFeatureAggregator); they are honoured, so the forward bits are model.forward's for such an input too
    stats = None if x.requires_grad else getattr(x, "_gn_stats", None)
    v = U.to_channel_last(x) if x.requires_grad else U.stored_volume(x)
    if v.shape[-1] % 16 != 0:                     # (the gradient of the zero pads is dropped here: F.pad's backward is a slice)
        v, stats = F.pad(v, (0, U.stored_channels(v.shape[-1]) - v.shape[-1])), None
    model.check_input(v)
    feats = []
    for enc in model.encoders:
        if enc.pooling is not None:
            v, stats = _pool(v)
        dc = enc.basic_module
        v, stats = _conv(dc.SingleConv1, v, None, stats, None, arith)
        v, stats = _conv(dc.SingleConv2, v, None, stats, None, arith)
        feats.insert(0, (v, stats))
    for dec, (skip, skip_stats) in zip(model.decoders, feats[1:]):
        dc = dec.basic_module
        v, stats = _conv(dc.SingleConv1, skip, v, skip_stats, stats, arith)
        v, stats = _conv(dc.SingleConv2, v, None, stats, None, arith)
    # the final 1x1x1 convolution: a linear block over the rows of stored channels (FinalConv1x1.run's launch on the same pack)
    fc = model.final_conv
    wp, b, k = fc.packed()
    y = _LinearBlock.apply(v.reshape(-1, v.shape[-1]), fc.weight, fc.bias, None, None, (wp, b, None, None, k), False, None, fc, 0)
    return y.reshape(*v.shape[:-1], fc.out_channels).permute(0, 4, 1, 2, 3)


# ------------------------------------------------------------------------------------------------ the MLP blocks
class _LinearBlock(torch.autograd.Function):
    """one block r = act(x W^T + b), y = r * sc + sh of an MLPStack, a bare HipLinear or the UNet's final 1x1x1 convolution.  layer = (wp, b, sc, sh,
    k): the forward's packs of the parameters, built at their present versions; wp[:, :k] is the weight as the kernels read it (the final convolution's
    over its STORED input channels, zero columns on the pads).  weight / bias / gamma / beta are the module's own parameters: they are saved, so the
    backward differentiates the parameters the forward used and an in-place update in between is an autograd version error.  bn: the BatchNorm module
    (its running statistics are data, read at the forward) or None; owner: the module whose ParamCache keeps the transposed weight pack."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, layer, relu, bn, owner, idx):
        wp, b, sc, sh, k = layer
        if x.shape[1] != k:
            raise ValueError(f"{type(owner).__name__}: input of {x.shape[1]} channels, expected {k}")
        r = ops.linear(x, wp, b, None, None, relu=relu, K=k)          # the epilogue apart: r is what the mask and the scale gradient need
        y = r if sc is None else ops.row_affine(r, sc, sh)
        ctx.save_for_backward(x, r if relu else None, weight, bias, gamma, beta)
        ctx.wp, ctx.k, ctx.sc, ctx.owner, ctx.idx = wp, k, sc, owner, idx
        if bn is not None:
            ctx.mean = bn.running_mean.detach().double()
            ctx.inv = 1.0 / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, r, weight, bias, gamma, beta = ctx.saved_tensors
        need = ctx.needs_input_grad
        n, k = weight.shape[0], ctx.k                # k: the width the kernels read (the final convolution's stored input channels)
        k_real = weight[0].numel()                    # the parameter's own input width: (n, k_real) or (n, k_real, 1, 1, 1)
        g, sums = ops.linear_act_bwd(ops.fp32_rows(grad_y, "grad_y", cols=n), r, ctx.sc)
        dx = dw = db = dgamma = dbeta = None
        if need[0]:
            dx = ops.linear(g, _wt_pack(ctx, weight), K=n)
        if need[1]:
            # (over the stored width; a channel-padded input's pad columns multiply exact zeros and reach no parameter)
            dw = ops.linear_bwd_weight(g, x, K=k)[:, :k_real].reshape(weight.shape)
        if bias is not None and need[2]:
            db = sums[0].float()
        if gamma is not None and need[3]:
            dgamma = ((sums[2] - ctx.mean * sums[1]) * ctx.inv).float()
        if beta is not None and need[4]:
            dbeta = sums[1].float()
        return dx, dw, db, dgamma, dbeta, None, None, None, None, None


def _wt_pack(ctx, weight):
    """the transposed weight pack of a block's dX = g W.  (The saved weight IS the module's at the forward's version -- unpacking it has checked that -- so
    the generation-keyed cache holds its pack, and ctx.wp, the forward's pack of it, holds its values.)"""
    return param_cache(ctx.owner, "_grad_packs").get(generation(ctx.owner), ("wt", ctx.idx), lambda: pack_wb(ctx.wp[:, :ctx.k].t().contiguous(), None)[0])


def _bn_update_buffers(bn, mean, m2, M):
    """nn.BatchNorm1d's in-place update of a training module's buffers from the batch's fp64 column mean and m2 = sum (r - mean)^2 over M rows: the
    UNBIASED variance m2 / (M - 1) goes into running_var; the factor is momentum, or 1 / num_batches_tracked (after its increment) under momentum=None"""
    with torch.no_grad():
        bn.num_batches_tracked.add_(1)
        f = bn.momentum if bn.momentum is not None else 1.0 / bn.num_batches_tracked.double()
        bn.running_mean.copy_((1.0 - f) * bn.running_mean.double() + f * mean)
        bn.running_var.copy_((1.0 - f) * bn.running_var.double() + f * (m2 / (M - 1)))


def _bn_bwd_coef(gamma, mean, inv, s_dy, s_dyr, M):
    """fp64, per column: the batch mean and inverse standard deviation, S_dy = sum_m dy, S_dyr = sum_m dy * r -> (dgamma, coef [3][N] = (a, b, c)) with
    the gradient at the ReLU's output a * dy + b * r + c (DESIGN.md "Train-mode BatchNorm"; dbeta is S_dy)"""
    dgamma = (s_dyr - mean * s_dy) * inv
    a = gamma.detach().double() * inv
    b = -a * inv * dgamma / M
    c = -a * s_dy / M - b * mean
    return dgamma, torch.stack((a, b, c))


def _batch_stats_forward(x, wp, b, k, bn):
    """one block under batch statistics: r = relu(x W^T + b), its column moments (gn_col_moments), y = gn_row_affine(r, sc, sh) with the batch mean and
    biased variance folded as fold_batchnorm folds the running ones (fp64, each of sc / sh rounded once), then the buffer update.  -> (r, y, mean, inv):
    the statistics in fp64"""
    r = ops.linear(x, wp, b, None, None, relu=True, K=k)
    M = r.shape[0]
    mean, m2 = ops.col_moments(r)
    inv = 1.0 / torch.sqrt(m2 / M + bn.eps)
    sc = bn.weight.detach().double() * inv
    sh = bn.bias.detach().double() - mean * sc
    y = ops.row_affine(r, sc.float().contiguous(), sh.float().contiguous())
    _bn_update_buffers(bn, mean, m2, M)
    return r, y, mean, inv


class _BatchStatsBlock(torch.autograd.Function):
    """one block r = relu(x W^T + b), y = BatchNorm(r) in training mode (DESIGN.md "Train-mode BatchNorm").  The backward reads the batch mean and inverse
    standard deviation the forward captured (fp64, on ctx), never the running buffers: their in-place update neither raises nor changes the gradient.
    The parameters are saved, as _LinearBlock saves them."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, wp, b, k, bn, owner, idx):
        if x.shape[1] != k:
            raise ValueError(f"{type(owner).__name__}: input of {x.shape[1]} channels, expected {k}")
        r, y, ctx.mean, ctx.inv = _batch_stats_forward(x, wp, b, k, bn)
        ctx.save_for_backward(x, r, weight, bias, gamma, beta)
        ctx.wp, ctx.k, ctx.owner, ctx.idx = wp, k, owner, idx
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, r, weight, bias, gamma, beta = ctx.saved_tensors
        need = ctx.needs_input_grad
        n, M = weight.shape[0], r.shape[0]
        dy = ops.fp32_rows(grad_y, "grad_y", cols=n)
        s_dy, s_dyr = ops.col_dots(dy, r)
        dgamma, coef = _bn_bwd_coef(gamma, ctx.mean, ctx.inv, s_dy, s_dyr, M)
        g, sum_g = ops.bn_train_bwd(dy, r, coef)
        dx = ops.linear(g, _wt_pack(ctx, weight), K=n) if need[0] else None
        dw = ops.linear_bwd_weight(g, x, K=ctx.k).reshape(weight.shape) if need[1] else None
        db = sum_g.float() if bias is not None and need[2] else None
        return dx, dw, db, dgamma.float() if need[3] else None, s_dy.float() if need[4] else None, None, None, None, None, None, None


def _needs_grad(module, x):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters()))


def _fp32_features(x, who):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise TypeError(f"{who}: expected torch.float32 features (..., C), got {getattr(x, 'dtype', type(x).__name__)}")
    return x


def _batch_stats_layers(stack):
    """the packs of a stack that holds a training BatchNorm: (wp, b, sc, sh, k) per block with (sc, sh) the folded running statistics of the EVAL-mode
    BatchNorms only (None for a training one: its buffers change at every call and are not read).  Its generation follows exactly the tensors it
    reads -- the parameters and the eval-mode buffers -- and the modes."""
    bns = [block[2] if len(block) > 2 else None for block in stack]
    read = list(stack.parameters()) + [t for bn in bns if bn is not None and not bn.training for t in (bn.running_mean, bn.running_var)]
    gen = generation(stack, tuple(bn is not None and bn.training for bn in bns), tensors=read)

    def build():
        layers = []
        for block, bn in zip(stack, bns):
            sc, sh = (None, None) if bn is None or bn.training else fold_batchnorm(bn)
            layers.append(pack_linear(block[0])[:2] + (sc, sh, block[0].in_features))
        return layers
    return param_cache(stack, "_grad_batch_stats_packs").get(gen, "layers", build)


def mlp(stack, x, batch_stats=False):
    """``MLPStack.forward``'s contract -- x fp32 (..., C) -> (..., C') through [Linear, ReLU, BatchNorm] blocks -- differentiable in x and in every Linear
    weight / bias and BatchNorm weight / bias of the stack.

    batch_stats=False: eval-mode BatchNorm, the running statistics are data.  Each block runs gn_linear with the ReLU and WITHOUT the BatchNorm epilogue,
    keeps x and r, and applies the epilogue's own fmul / fadd as gn_row_affine: the bits are ``stack(x)``'s, and the mask is the forward's own r > 0
    (y = r * sc + sh cannot be inverted).  Backward: csrc/linear_grad.hip, dX = gn_linear on the transposed pack.  A stack with a BatchNorm in training
    mode raises NotImplementedError (the forward folds the running statistics whatever the mode, so that gradient would silently be the wrong one; a
    fresh module is in training mode -- call .eval(), or pass batch_stats=True).  Under torch.no_grad(), or when nothing requires a gradient, this is
    ``stack(x)``'s launches and nothing is saved.

    batch_stats=True: torch's per-module rule.  A BatchNorm in training mode normalises with the mean and biased variance of its input over ALL rows
    (every leading dimension flattened, as PointBatchNorm1D does), the gradient flows through both statistics, and its running_mean / running_var /
    num_batches_tracked are updated in place as nn.BatchNorm1d updates them -- under no_grad too, where nothing is saved.  A BatchNorm in eval mode in
    the same stack keeps the path above.  Refused before any launch: track_running_stats=False (NotImplementedError), fewer than 2 rows (ValueError)."""
    if not isinstance(stack, MLPStack):
        raise TypeError(f"mlp: expected a components.mlp.MLPStack, got {type(stack).__name__}")
    _fp32_features(x, "mlp")
    training = [len(block) > 2 and block[2].training for block in stack]
    if any(training) and not batch_stats:
        raise NotImplementedError("mlp: train-mode BatchNorm has no gradient here (the forward folds the running statistics): call .eval() on the stack, "
                                  "or pass batch_stats=True to normalise with the batch's own statistics")
    if any(training):
        rows = x.numel() // x.shape[-1] if x.shape[-1] else 0
        for block, t in zip(stack, training):
            if t and (not block[2].track_running_stats or block[2].running_mean is None or block[2].running_var is None):
                raise NotImplementedError("mlp: a training BatchNorm with track_running_stats=False (no running buffers) is not supported")
            if t and rows < 2:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    grad = _needs_grad(stack, x)
    if not grad and not any(training):
        with torch.no_grad():
            return stack(x)
    lead = x.shape[:-1]
    h = ops.fp32_rows(x.reshape(-1, x.shape[-1]), "x")
    layers = _batch_stats_layers(stack) if any(training) else stack.packed()
    for i, (block, layer, t) in enumerate(zip(stack, layers, training)):
        lin, bn = block[0], block[2] if len(block) > 2 else None
        wp, b, sc, sh, k = layer
        if not grad:
            with torch.no_grad():
                h = _batch_stats_forward(h, wp, b, k, bn)[1] if t else ops.linear(h, wp, b, sc, sh, relu=True, K=k)
        elif t:
            h = _BatchStatsBlock.apply(h, lin.weight, lin.bias, bn.weight, bn.bias, wp, b, k, bn, stack, i)
        else:
            h = _LinearBlock.apply(h, lin.weight, lin.bias, None if bn is None else bn.weight, None if bn is None else bn.bias, layer, True, bn, stack, i)
    return h.reshape(*lead, h.shape[-1])


def linear(hip_linear, x, relu=False):
    """``HipLinear.forward``'s contract -- x fp32 (..., K) -> (..., N), optionally with the fused ReLU -- differentiable in x, weight and bias"""
    if not isinstance(hip_linear, HipLinear):
        raise TypeError(f"linear: expected a components.mlp.HipLinear, got {type(hip_linear).__name__}")
    _fp32_features(x, "linear")
    if not _needs_grad(hip_linear, x):
        with torch.no_grad():
            return hip_linear(x, relu=relu)
    lead = x.shape[:-1]
    h = ops.fp32_rows(x.reshape(-1, x.shape[-1]), "x")
    wp, b, k = hip_linear.packed()
    h = _LinearBlock.apply(h, hip_linear.weight, hip_linear.bias, None, None, (wp, b, None, None, k), bool(relu), None, hip_linear, 0)
    return h.reshape(*lead, h.shape[-1])


def implicit_decode(decoder, features_grid, query_points, batch_stats=False):
    """``ImplicitWNFDecoder.forward``'s contract -- features_grid (B, C, D, H, W), query_points (B, M, 3) in [0, 1] -> (B, M, out) -- as the unfused
    chain ``grid_sample_points`` -> ``mlp(decoder.mlp, .)``, differentiable in the volume, the queries and the decoder's parameters.  The fused and
    split-operand decoder kernels stay inference-only.  batch_stats: ``mlp``'s keyword (the statistics run over all B * M query rows)."""
    from .networks.conv_implicit_wnf import ImplicitWNFDecoder
    if not isinstance(decoder, ImplicitWNFDecoder):
        raise TypeError(f"implicit_decode: expected a networks.conv_implicit_wnf.ImplicitWNFDecoder, got {type(decoder).__name__}")
    return mlp(decoder.mlp, grid_sample_points(features_grid, query_points.float()), batch_stats=batch_stats)


# ------------------------------------------------------------------------------------------------ the losses
def _weighted_mean_loss(sums, col, weights, counts):
    """sum_s weights[s] * (sums[s][col] / counts[s]) in fp64 on the device, left to right: validation_metrics' own expression"""
    dev = sums.device
    terms = torch.tensor([float(w) for w in weights], dtype=torch.float64, device=dev) * \
        (sums[:, col] / torch.tensor([float(c) for c in counts], dtype=torch.float64, device=dev))
    total = terms[0]
    for s in range(1, terms.shape[0]):
        total = total + terms[s]
    return total


class _NocsBinLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bins, mirror_axis, weights, gts, *logits):
        sets = list(zip(logits, gts))
        sums = ops.nocs_bin_metrics(sets, bins, mirror_axis)
        counts = [lg.shape[0] * 3 for lg in logits]
        loss = _weighted_mean_loss(sums, 0, weights, counts)
        if mirror_axis is not None:                # the whole batch takes the smaller weighted loss (plain when equal)
            loss = torch.minimum(loss, _weighted_mean_loss(sums, 1, weights, counts))
        ctx.save_for_backward(sums, *logits)
        ctx.gts, ctx.cfg = gts, (bins, mirror_axis, weights)
        ctx.mark_non_differentiable(sums)
        return loss.float(), sums

    @staticmethod
    def backward(ctx, grad_loss, _):
        sums, *logits = ctx.saved_tensors
        bins, mirror_axis, weights = ctx.cfg
        grads = ops.nocs_bin_loss_bwd(list(zip(logits, ctx.gts)), bins, mirror_axis, sums, weights, grad_loss.float())
        return (None, None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[4:]))


def nocs_bin_loss(sets, bins, mirror_axis=None, weights=None):
    """The binned NOCS loss of PointNet2NOCS (cross entropy at VirtualGrid's target bins) over 1..8 row sets sets = [(logits (N, >= bins*3) fp32, gt
    (N, 3))]: loss = sum_s weights[s] * CE_s / (3 n_s); with a mirror_axis the whole batch takes the mirrored targets iff that weighted loss is strictly
    smaller (``validation_metrics``' rule).  -> (loss, sums): loss a device fp32 scalar that autograd tracks, built from the fp64 sums as
    ``validation_metrics`` builds its "loss" and cast once; sums the detached (nsets, 4) fp64 result of gn_nocs_bin_metrics.  Forward: that kernel,
    unchanged.  Backward: gn_nocs_bin_loss_bwd -- the branch is decided on the device from the sums, nothing is read back."""
    weights = [1.0] * len(sets) if weights is None else [float(w) for w in weights]
    if len(weights) != len(sets):
        raise ValueError(f"nocs_bin_loss: {len(sets)} sets but {len(weights)} weights")
    for logits, _ in sets:
        _fp32_features(logits, "nocs_bin_loss")
    gts = tuple(gt.detach() for _, gt in sets)
    return _NocsBinLoss.apply(int(bins), mirror_axis, tuple(weights), gts, *[lg for lg, _ in sets])


class _ValueLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kinds, weights, targets, *preds):
        segs = [(p, t) + k for p, t, k in zip(preds, targets, kinds)]
        sums = ops.value_losses(segs)
        best = torch.where(torch.tensor([k[1] for k in kinds], device=sums.device), torch.minimum(sums[:, 0], sums[:, 1]), sums[:, 0])
        loss = _weighted_mean_loss(best[:, None], 0, weights, [p.numel() for p in preds])
        ctx.save_for_backward(sums, *preds)
        ctx.targets, ctx.cfg = targets, (kinds, weights)
        ctx.mark_non_differentiable(sums)
        return loss.float(), sums

    @staticmethod
    def backward(ctx, grad_loss, _):
        sums, *preds = ctx.saved_tensors
        kinds, weights = ctx.cfg
        grads = ops.value_losses_bwd([(p, t) + k for p, t, k in zip(preds, ctx.targets, kinds)], sums, weights, grad_loss.float())
        return (None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:]))


def value_loss(segments, weights=None):
    """Mean-reduced element-wise losses over 1..8 segments = [(pred, target, kind[, mirror])], kind "l2" | "smooth_l1" | "bce_logits" (torch's
    F.mse_loss / smooth_l1_loss / binary_cross_entropy_with_logits): loss = sum_s weights[s] * sum_s / count_s, where a mirrored segment of (M, 3)
    rows takes the sum against its x-mirrored target when that is strictly smaller (MirrorMSELoss, decided per segment).  "row_norm" is a metric, not
    a loss: ValueError.  -> (loss, sums) as ``nocs_bin_loss``: forward gn_value_losses, unchanged; backward gn_value_losses_bwd, the mirror choice
    taken on the device."""
    weights = [1.0] * len(segments) if weights is None else [float(w) for w in weights]
    if len(weights) != len(segments):
        raise ValueError(f"value_loss: {len(segments)} segments but {len(weights)} weights")
    kinds = []
    for seg in segments:
        if seg[2] == "row_norm":
            raise ValueError("value_loss: row_norm is a metric, not a loss: it has no gradient")
        if seg[2] not in ("l2", "smooth_l1", "bce_logits"):
            raise ValueError(f"value_loss: loss kind {seg[2]!r}: expected one of 'l2', 'smooth_l1', 'bce_logits'")
        _fp32_features(seg[0], "value_loss")
        kinds.append((seg[2], bool(seg[3]) if len(seg) > 3 else False))
    return _ValueLoss.apply(tuple(kinds), tuple(weights), tuple(seg[1].detach() for seg in segments), *[seg[0] for seg in segments])
