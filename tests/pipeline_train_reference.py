"""The torch restatement of the second stage's training step (tests/test_gpu_train_pipeline.py, tests/test_train_pipeline_host.py), built from
tests/grad_reference.py (r_layer, r_sample, _first_max) and tests/train_reference.py (VALUE_LOSS).  Plain torch at any dtype on the CPU; a plain module,
imported by its siblings; it holds no test.

Written from the model's documented contract: rows -> [Linear -> ReLU -> BatchNorm1d] blocks -> scatter (mean | sum | max | min, empty cells 0) into
(B, C, G, G, G) -> 'gcr' layers (GroupNorm -> Conv3d 3x3x3 -> ReLU), max_pool3d(2), nearest upsampling + concat, a 1x1x1 convolution ->
F.grid_sample(..., 'bilinear', 'border', align_corners=True) -> the decoders' blocks -> F.mse_loss / smooth_l1_loss / binary_cross_entropy_with_logits,
weighted.  The rows the aggregator reads and every point's cell (ops.grid_features' results) are data, handed in.

Selections, the project's convention: the ReLU masks are taken from the HIP forward -- `record_second_stage` captures them -- so both sides differentiate
the same piecewise-linear map; the max winners (scatter max / min, max-pool) are each side's own.  Without masks the restatement forms its own ReLUs."""
import contextlib

import torch
import torch.nn.functional as F

from grad_reference import _first_max, r_layer, r_sample
from train_reference import VALUE_LOSS


# ------------------------------------------------------------------------------------------------ what the HIP forward decided
@contextlib.contextmanager
def record_second_stage():
    """while active: every gn_linear call with a ReLU and no folded epilogue leaves its output r (the MLP blocks, in execution order: the masks, and the
    rows a training BatchNorm saw), every SingleConv.run the mask y > 0 of its real output channels (NCDHW, CPU).  Wrap the second stage only: the frozen
    first stage's lin1 would leave an r as well."""
    from garmentnets_amd import ops
    from garmentnets_amd.components import unet3d as U
    rec = {"r": [], "conv": []}
    linear, run = ops.linear, U.SingleConv.run

    def rec_linear(x, w, bias=None, bn_scale=None, bn_shift=None, relu=False, out=None, K=None):
        y = linear(x, w, bias, bn_scale, bn_shift, relu=relu, out=out, K=K)
        if relu and bn_scale is None:
            rec["r"].append(y.detach().clone())
        return y

    def rec_run(self, *args, **kw):
        res = run(self, *args, **kw)
        rec["conv"].append((res[0][..., :self.conv.out_channels] > 0).permute(0, 4, 1, 2, 3).cpu())
        return res
    ops.linear, U.SingleConv.run = rec_linear, rec_run
    try:
        yield rec
    finally:
        ops.linear, U.SingleConv.run = linear, run


# ------------------------------------------------------------------------------------------------ the operators
def r_scatter(src, flat, cells, reduce):
    """torch_scatter.scatter(src (N, C), flat (N,), dim 0, dim_size cells, reduce) -> (cells, C), empty cells 0; max / min: the first maximum of a cell
    (written out over the occupied cells: no reliance on a scatter kernel's tie rule)"""
    flat = flat.long()
    uniq, inv = torch.unique(flat, return_inverse=True)
    member = inv[None, :] == torch.arange(uniq.numel())[:, None]                     # (occupied cells, N)
    if reduce in ("sum", "add", "mean"):
        red = member.to(src.dtype) @ src
        if reduce == "mean":
            red = red / member.sum(1, keepdim=True).to(src.dtype)
    elif reduce in ("max", "min"):
        vals = src[None].expand(uniq.numel(), *src.shape)
        sel = _first_max(vals.detach() if reduce == "max" else -vals.detach(), member[:, :, None].expand_as(vals), 1)
        red = (vals * sel.to(src.dtype)).sum(1)
    else:
        raise ValueError(reduce)
    return torch.zeros((cells, src.shape[1]), dtype=src.dtype).index_copy(0, uniq, red)


def r_unet(model, P, x, masks=None, prefix=""):
    """Abstract3DUNet.forward in 'gcr' order on x (B, C, D, H, W); masks: the ReLU selections per layer in execution order, None: its own.  The
    max-pool winners are its own either way."""
    masks = None if masks is None else iter(masks)

    def double_conv(name, dc, x0, x1=None):
        for k in ("SingleConv1", "SingleConv2"):
            gn, n = getattr(dc, k).groupnorm, f"{prefix}{name}.basic_module.{k}"
            x0 = r_layer(x0, x1, P[n + ".conv.weight"], P[n + ".groupnorm.weight"], P[n + ".groupnorm.bias"], gn.num_groups, gn.eps,
                         mask=None if masks is None else next(masks).to(x0.dtype))
            x1 = None
        return x0
    feats = []
    for i, enc in enumerate(model.encoders):
        if i > 0:
            x = F.max_pool3d(x, 2)
        x = double_conv(f"encoders.{i}", enc.basic_module, x)
        feats.insert(0, x)
    for i, dec in enumerate(model.decoders):
        x = double_conv(f"decoders.{i}", dec.basic_module, feats[i + 1], x)
    return F.conv3d(x, P[prefix + "final_conv.weight"], P[prefix + "final_conv.bias"])


HEADS = (("volume_decoder", "volume_query_points"), ("surface_decoder", "surf_query_points"), ("mc_surface_decoder", "mc_surf_query_points"))


class Restated:
    """The second stage of ConvImplicitWNFPipeline and its loss in plain torch at `dtype`.  model: the CPU module (structure, hyper-parameters); P: name ->
    parameter (leaf, dtype) under the model's own names; buffers: name -> running statistic (data); training: BatchNorm on the batch's statistics;
    masks: (the r > 0 of every MLP block, the y > 0 of every UNet layer), each in execution order, or None"""

    def __init__(self, model, P, buffers, dtype, training, masks=None):
        self.model, self.P, self.B, self.dtype, self.training = model, P, buffers, dtype, training
        self.mlp_masks = None if masks is None else iter(masks[0])
        self.conv_masks = None if masks is None else masks[1]

    def mlp(self, prefix, stack, h):
        for i, block in enumerate(stack):
            p = f"{prefix}.{i}"
            h = F.linear(h, self.P[p + ".0.weight"], self.P[p + ".0.bias"])
            h = F.relu(h) if self.mlp_masks is None else h * next(self.mlp_masks).to(self.dtype)
            if len(block) > 2:
                bn = block[2]
                if self.training:
                    h = F.batch_norm(h, None, None, self.P[p + ".2.weight"], self.P[p + ".2.bias"], True, 0.0, bn.eps)
                else:
                    h = F.batch_norm(h, self.B[p + ".2.running_mean"].to(self.dtype), self.B[p + ".2.running_var"].to(self.dtype), self.P[p + ".2.weight"],
                                     self.P[p + ".2.bias"], False, 0.0, bn.eps)
        return h

    def predictions(self, rows, flat, batch):
        """rows (N, C0), flat (N,): ops.grid_features' results (data) -> [the heads' outputs (B, M, out)] in the model's order"""
        m, dt = self.model, self.dtype
        agg = m.volume_agg
        nb = batch.volume_query_points.shape[0]
        g = agg.grid_shape
        f = self.mlp("volume_agg.local_nn", agg.local_nn, rows.to(dt))
        vol = r_scatter(f, flat, nb * g[0] * g[1] * g[2], agg.reduce_method).view(nb, *g, f.shape[1]).permute(0, 4, 1, 2, 3)
        out = r_unet(m.unet_3d.abstract_3d_unet, self.P, vol, self.conv_masks, "unet_3d.abstract_3d_unet.")
        preds = []
        for name, queries in HEADS:
            dec = getattr(m, name, None)
            if dec is not None:
                q = getattr(batch, queries).to(dt)
                s = r_sample(out, q)
                preds.append(self.mlp(name + ".mlp", dec.mlp, s.reshape(-1, s.shape[-1])).reshape(q.shape[0], q.shape[1], -1))
        return preds

    def loss(self, rows, flat, batch):
        """the weighted loss of infer: volume (BCE-with-logits when volume_classification, else loss_type), surface (loss_type), mc surface (BCE)"""
        m, dt = self.model, self.dtype
        preds = self.predictions(rows, flat, batch)
        pv = preds[0].reshape(preds[0].shape[:-1])
        total = m.volume_loss_weight * VALUE_LOSS["bce_logits" if m.volume_classification else m.loss_type](pv, batch.gt_volume_value.to(dt))
        total = total + m.surface_loss_weight * VALUE_LOSS[m.loss_type](preds[1], batch.gt_sim_points.to(dt))
        if m.mc_surface_loss_weight > 0:
            total = total + m.mc_surface_loss_weight * VALUE_LOSS["bce_logits"](preds[2], batch.is_query_point_on_surf.to(dt))
        return total
