"""PointNet2NOCS -- API twin of the reference's networks/pointnet2_nocs.py:58-195.

Same constructor kwargs, sub-module names (``sa1_module`` ... ``global_lin2``: the checkpoint schema), ``forward(data)``
result keys and ``logits_to_nocs`` / ``get_virtual_grid`` helpers, and ``validation_metrics`` (the metric dict of the
reference's ``infer``, :257-440, without its logging).  ``forward`` is the fused inference path.  ``training_step`` /
``training_metrics`` / ``configure_optimizers`` are thin methods over garmentnets_amd.train (the differentiable forward, the HIP
loss gradients, optim.FusedAdam), imported lazily: the inference path imports none of the differentiable bindings.  ``vis_batch`` renders the
reference's monitor images on the device (garmentnets_amd.visualize).  All arithmetic runs in HIP kernels (garmentnets_amd.ops), with one exception in training mode: the reference's four
dropouts (present iff ``dropout=True``) are torch.nn.functional.dropout (train.py's docstring).
"""
import torch
from torch import nn

from .. import ops
from ..components.gridding import VirtualGrid
from ..components.mlp import MLP, HipLinear
from ..components.pointnet2 import FPModule, GlobalSAModule, SAModule, Segments


class PointNet2NOCS(nn.Module):
    def __init__(self, feature_dim, batch_norm, dropout, sa1_ratio, sa1_r, sa2_ratio, sa2_r, fp3_k, fp2_k, fp1_k,
                 symmetry_axis=None, nocs_bins=None, learning_rate=1e-4, nocs_loss_weight=1, grip_point_loss_weight=1,
                 vis_per_items=0, max_vis_per_epoch_train=0, max_vis_per_epoch_val=0, batch_size=None):
        super().__init__()
        self.hparams = dict(feature_dim=feature_dim, batch_norm=batch_norm, dropout=dropout, sa1_ratio=sa1_ratio, sa1_r=sa1_r,
                            sa2_ratio=sa2_ratio, sa2_r=sa2_r, fp3_k=fp3_k, fp2_k=fp2_k, fp1_k=fp1_k, symmetry_axis=symmetry_axis,
                            nocs_bins=nocs_bins, learning_rate=learning_rate, nocs_loss_weight=nocs_loss_weight,
                            grip_point_loss_weight=grip_point_loss_weight, vis_per_items=vis_per_items,
                            max_vis_per_epoch_train=max_vis_per_epoch_train, max_vis_per_epoch_val=max_vis_per_epoch_val)
        self.sa1_module = SAModule(sa1_ratio, sa1_r, MLP([3 + 3, 64, 64, 128], batch_norm=batch_norm))
        self.sa2_module = SAModule(sa2_ratio, sa2_r, MLP([128 + 3, 128, 128, 256], batch_norm=batch_norm))
        self.sa3_module = GlobalSAModule(nn=MLP([256 + 3, 256, 512, 1024], batch_norm=batch_norm))
        self.fp3_module = FPModule(k=fp3_k, nn=MLP([1024 + 256, 256, 256], batch_norm=batch_norm))
        self.fp2_module = FPModule(k=fp2_k, nn=MLP([256 + 128, 256, 128], batch_norm=batch_norm))
        self.fp1_module = FPModule(k=fp1_k, nn=MLP([128 + 3, 128, 128, 128], batch_norm=batch_norm))
        output_dim = 3 if nocs_bins is None else nocs_bins * 3
        self.lin1 = HipLinear(128, 128)
        self.lin2 = HipLinear(128, feature_dim)
        self.lin3 = HipLinear(feature_dim, output_dim)
        self.global_lin1 = HipLinear(1024, 1024)
        self.global_lin2 = HipLinear(1024, output_dim)
        self.nocs_bins = nocs_bins
        self.symmetry_axis = symmetry_axis
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.nocs_loss_weight = nocs_loss_weight
        self.grip_point_loss_weight = grip_point_loss_weight
        self.vis_per_items = vis_per_items
        self.max_vis_per_epoch_train = max_vis_per_epoch_train
        self.max_vis_per_epoch_val = max_vis_per_epoch_val

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location="cpu", **overrides):
        """a standalone PointNet2NOCS checkpoint {'state_dict', 'hyper_parameters'} (train_pointnet2.py's), without Lightning"""
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
        return self.lin1.weight.device

    def set_self_loop_scope(self, scope):
        """"batch" (default; PyG's literal PointConv rule on a batched graph) or "example" (every garment of a batch gets its batch-of-one
        result: what the reference's predict.py, which asserts batch_size == 1, produces) -- components/pointnet2.py PointConv"""
        if scope not in ("batch", "example"):
            raise ValueError(f"self_loop_scope={scope!r}")
        self.sa1_module.conv.self_loop_scope = self.sa2_module.conv.self_loop_scope = scope
        return self

    def forward(self, data, seg=None):
        """data: .x (N,3) rgb, .pos (N,3), .batch (N,) sorted int64 [, .sizes host list] -- eval mode (dropout = identity).
        seg: the batch's Segments when the caller already has them (ConvImplicitWNFPipeline.pointnet2_forward: sizes travel with the call,
        nothing about a batch is parked on the shared module)"""
        if seg is None:
            sizes = data._sizes if hasattr(data, "_sizes") else getattr(data, "sizes", None)
            seg = Segments.of(data.batch, sizes)
        x = data.x.float().contiguous()
        pos = data.pos.float().contiguous()
        sa0 = (x, pos, seg)
        sa1 = self.sa1_module(*sa0)
        sa2 = self.sa2_module(*sa1)
        sa3 = self.sa3_module(*sa2)
        fp3 = self.fp3_module(*sa3, *sa2)
        fp2 = self.fp2_module(*fp3, *sa1)
        h, _, _ = self.fp1_module(*fp2, *sa0)
        h = self.lin1(h, relu=True)
        features = self.lin2(h)
        logits = self.lin3(features)
        global_feature = sa3[0]
        g = self.global_lin1(torch.relu(global_feature))
        global_logits = self.global_lin2(g)
        return {
            "per_point_features": features,
            "per_point_logits": logits,
            "per_point_batch_idx": data.batch,
            "global_logits": global_logits,
            "global_feature": global_feature,
        }

    # -- training (garmentnets_amd/train.py, imported on first use) --------------------------------------------
    def training_step(self, batch, batch_idx=None):
        """the reference's metrics['loss'] of one batch: a device scalar with a graph through every parameter"""
        from .. import train
        return train.training_step(self, batch, batch_idx)

    def training_metrics(self, batch):
        """validation_metrics' five keys for the model AS IT STANDS (training-mode BatchNorm and dropout included), detached python floats,
        from the sums of the loss kernel: one forward"""
        from .. import train
        return train.training_metrics(self, batch)

    def configure_optimizers(self):
        from ..optim import FusedAdam
        return FusedAdam(self.parameters(), lr=self.learning_rate, modules=self)

    def logits_to_nocs(self, logits):
        if self.nocs_bins is None:
            return logits
        lg = logits.reshape(-1, self.nocs_bins * 3)
        _, _, nocs = ops.nocs_head(lg, self.nocs_bins)
        return nocs.reshape(logits.shape[:-1] + (3,)) if logits.dim() == 2 else nocs.reshape(3)

    def get_virtual_grid(self):
        return VirtualGrid(lower_corner=(0, 0, 0), upper_corner=(1, 1, 1), grid_shape=(self.nocs_bins,) * 3, batch_size=1,
                           device=self.device, int_dtype=torch.int64, float_dtype=torch.float32)

    # -- monitors (garmentnets_amd/visualize.py) -------------------------------------------------------------
    def vis_batch(self, batch, batch_idx, result, is_train=False, img_size=256, backend="device"):
        """the reference's vis_batch (pointnet2_nocs.py:203-255) -> {label: (2 S or S, 2 S, 4) fp32 image}, labels train_<vis_idx> / val_<vis_idx>: per
        selected garment (get_vis_idxs over vis_per_items / max_vis_per_epoch_* / batch_size) the NOCS pair with the ground-truth, the predicted
        (the prediction at the point nearest the gripper) and the global head's grip point over it, above the confidence pair of the x bins when
        the head has bins.  result: this model's forward of the batch; all images of the batch in one launch pair.  No garment selected: nothing
        is launched, nothing synchronises."""
        from .. import visualize as V
        picked = V.monitor_selection(self, batch_idx, batch.nocs_grip_point.shape[0], is_train)
        if not picked:
            return {}
        with torch.no_grad():
            logits, glogits = result["per_point_logits"].detach(), result["global_logits"].detach()
            if self.nocs_bins is None:
                pred, grip_nn, conf = logits, glogits, None
            else:
                _, conf, pred = ops.nocs_head(logits, self.nocs_bins)
                grip_nn = self.logits_to_nocs(glogits)
            rows = V.garment_rows(batch)
            specs = [s for i, _ in picked for s in V.nocs_monitor_specs(rows, i, batch, pred, grip_nn, conf)]
            images = V.render_batch(specs, img_size, backend)
        return dict(zip([label for _, label in picked], V.compose(images, len(specs) // len(picked))))

    # -- validation ----------------------------------------------------------------------------------------
    def validation_metrics(self, batch, result=None):
        """the metric dict of the reference's infer (pointnet2_nocs.py:257-440) as python floats: loss, nocs_loss, grip_point_loss,
        nocs_err_dist, grip_point_err_dist.  batch: .x, .pos, .batch, .y (N, 3) NOCS targets, .nocs_grip_point (B, 3).  result: this model's
        forward(batch) when the caller already has it.
          regression (nocs_bins None): MSE of the logits, MirrorMSELoss (min of the plain and the x-mirrored MSE) when symmetry_axis is set;
          bins, no symmetry axis: cross entropy at VirtualGrid's target bins, arg-max coordinates for the distances;
          bins and symmetry_axis: the same against the plain and the mirrored targets; the WHOLE batch takes the branch with the smaller
          weighted loss (plain when equal) and loss = that minimum."""
        if result is None:
            result = self(batch)
        logits, glogits = result["per_point_logits"], result["global_logits"]
        gt, ggt = batch.y, batch.nocs_grip_point
        n, b = gt.shape[0], ggt.shape[0]
        if self.nocs_bins is None:
            mirror = self.symmetry_axis is not None
            s = ops.value_losses([(logits, gt, "l2", mirror), (glogits, ggt, "l2", mirror), (logits, gt, "row_norm"), (glogits, ggt, "row_norm")])
            s = s.cpu().tolist()
            return self.metrics_from_sums(s[:2], n, b, dist=(s[2][0], s[3][0]))
        return self.metrics_from_sums(ops.nocs_bin_metrics([(logits, gt), (glogits, ggt)], self.nocs_bins, self.symmetry_axis).cpu().tolist(), n, b)

    def metrics_from_sums(self, s, n, b, dist=None):
        """the metric dict from the loss kernels' sums as python floats, for n points and b garments.  bins: s = gn_nocs_bin_metrics' (2, 4);
        regression: s = gn_value_losses' (2, 2) of the two l2 segments and dist = the two row-norm sums"""
        wn, wg = self.nocs_loss_weight, self.grip_point_loss_weight
        if self.nocs_bins is None:
            mirror = self.symmetry_axis is not None
            nocs = min(s[0][0], s[0][1]) if mirror else s[0][0]
            grip = min(s[1][0], s[1][1]) if mirror else s[1][0]
            nocs_loss, grip_loss = nocs / (n * 3), grip / (b * 3)
            return {"loss": wn * nocs_loss + wg * grip_loss, "nocs_loss": nocs_loss, "grip_point_loss": grip_loss,
                    "nocs_err_dist": dist[0] / n, "grip_point_err_dist": dist[1] / b}

        def branch(ce, err):
            nocs_loss, grip_loss = s[0][ce] / (n * 3), s[1][ce] / (b * 3)
            return {"loss": wn * nocs_loss + wg * grip_loss, "nocs_loss": nocs_loss, "grip_point_loss": grip_loss,
                    "nocs_err_dist": s[0][err] / n, "grip_point_err_dist": s[1][err] / b}

        plain = branch(0, 2)
        if self.symmetry_axis is None:
            return plain
        mirrored = branch(1, 3)
        final = dict(plain if plain["loss"] <= mirrored["loss"] else mirrored)
        final["loss"] = min(plain["loss"], mirrored["loss"])
        return final
