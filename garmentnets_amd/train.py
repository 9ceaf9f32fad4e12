"""The first stage's training step: PointNet2NOCS, its loss and Adam, as train_pointnet2.py runs them -- without Hydra, wandb or Lightning.

  pointnet2_nocs_forward(model, data)   PointNet2NOCS.forward's contract and result keys, composed of the differentiable operators of autograd.py
                                        (fps / ball_table / point_conv_max / global_max_pool / knn_interpolate / mlp / linear).  It honours every
                                        module's .training (a stack holding a training BatchNorm normalises with the batch's statistics and updates its
                                        buffers; an eval one folds the running statistics) and the SA modules' random_start, add_self_loops,
                                        self_loop_scope and max_num_neighbors.  A module that needs no gradient and holds no training BatchNorm runs
                                        its own inference forward: with the model in eval mode and under no_grad the result is forward's, bit for bit.
  loss_and_sums / metrics_from_sums     the reference's metrics['loss'] as a device scalar with a graph (autograd.nocs_bin_loss over the per-point and the
                                        global row set; autograd.value_loss with l2 in regression mode), and the five logged values from the same sums.
  STAGE                                 this stage as train_loop.py's loop reads it; train_step / training_step / training_metrics are the loop's, bound to it
  python -m garmentnets_amd.train       train_loop.run over the train subset of a dataset store: epochs, validate.py's loop on val after each, a csv and a
                                        checkpoint, the monitor images, one GPU or several (train_loop.py's docstring)

Real edges only.  Inside the two SA modules local_nn runs over the rows of real edges (slot_src >= 0) and not over the empty slots of the ball table:
BatchNorm statistics and the running buffers see exactly PyG's edge set, which is also what the fused inference kernel later applies them to.

Dropout is the one deliberate exception to "all arithmetic in HIP": the reference's four dropouts (dp1, dp2, global_dp1, global_dp2; p = 0.5, present
iff dropout=True) are torch.nn.functional.dropout on four small tensors, at the reference's positions, when the model is in training mode -- torch's
generator stream could not be matched by a kernel of ours anyway.

The second stage (ConvImplicitWNFPipeline behind this model, frozen) is garmentnets_amd/train_pipeline.py, named after the reference's script;
`--model pipeline` is refused here.

What stays out: a HIP dropout, a compacting gather kernel in place of the index_select / index_copy
around local_nn.
"""
import functools

import torch
import torch.nn.functional as F

from . import autograd as A
from . import ops
from . import train_loop as L
from . import validate
from .components.pointnet2 import Segments

METRIC_KEYS = ("loss", "nocs_loss", "grip_point_loss", "nocs_err_dist", "grip_point_err_dist")


# ------------------------------------------------------------------------------------------------ the differentiable forward
def _sa(module, x, pos, seg):
    nn_ = module.conv.local_nn
    if L.plain(nn_, x):
        with torch.no_grad():
            return module(x, pos, seg)
    idx = A.fps(pos, seg, module.ratio, random_start=module.random_start)
    cseg = Segments([ops.fps_count(n, module.ratio) for n in seg.sizes], pos.device)
    nbr, _ = A.ball_table(pos, idx, module.r, seg, cseg, module.max_num_neighbors)
    out = A.point_conv_max(x, pos, idx, nbr, lambda e: L.mlp(nn_, e), add_self_loops=module.conv.add_self_loops,
                           self_loop_scope=module.conv.self_loop_scope, batch=seg, batch_centre=cseg, real_edges=True)
    return out, pos[idx], cseg


def _global_sa(module, x, pos, seg):
    if L.plain(module.nn, x):
        with torch.no_grad():
            return module(x, pos, seg)
    out = A.global_max_pool(L.mlp(module.nn, torch.cat((x, pos), 1)), seg)
    return out, pos.new_zeros((seg.num, 3)), Segments([1] * seg.num, pos.device)


def _fp(module, x, pos, seg, x_skip, pos_skip, seg_skip):
    if L.plain(module.nn, x, x_skip):
        with torch.no_grad():
            return module(x, pos, seg, x_skip, pos_skip, seg_skip)
    h = A.knn_interpolate(x, pos, pos_skip, seg, seg_skip, k=module.k)
    if x_skip is not None:
        h = torch.cat((h, x_skip), 1)
    return L.mlp(module.nn, h), pos_skip, seg_skip


def _dropout(model, h):
    return F.dropout(h, p=0.5, training=True) if model.hparams["dropout"] and model.training else h


def pointnet2_nocs_forward(model, data, seg=None):
    """PointNet2NOCS.forward's contract and result keys, differentiable in every parameter (the module docstring)"""
    if seg is None:
        sizes = data._sizes if hasattr(data, "_sizes") else getattr(data, "sizes", None)
        seg = Segments.of(data.batch, sizes)
    x = data.x.float().contiguous()
    pos = data.pos.float().contiguous()
    sa0 = (x, pos, seg)
    sa1 = _sa(model.sa1_module, *sa0)
    sa2 = _sa(model.sa2_module, *sa1)
    sa3 = _global_sa(model.sa3_module, *sa2)
    fp3 = _fp(model.fp3_module, *sa3, *sa2)
    fp2 = _fp(model.fp2_module, *fp3, *sa1)
    h, _, _ = _fp(model.fp1_module, *fp2, *sa0)
    h = _dropout(model, A.linear(model.lin1, h, relu=True))
    features = _dropout(model, A.linear(model.lin2, h))
    logits = A.linear(model.lin3, features)
    global_feature = sa3[0]
    g = _dropout(model, torch.relu(global_feature))
    g = _dropout(model, A.linear(model.global_lin1, g))
    global_logits = A.linear(model.global_lin2, g)
    return {"per_point_features": features, "per_point_logits": logits, "per_point_batch_idx": data.batch, "global_logits": global_logits,
            "global_feature": global_feature}


# ------------------------------------------------------------------------------------------------ loss, metrics, step
def loss_and_sums(model, batch, result=None):
    """-> (loss, sums): the reference's metrics['loss'] of one batch as a device scalar with a graph, and the detached fp64 sums of the loss kernel
    (the metrics are formed from them: no second forward)"""
    if result is None:
        result = pointnet2_nocs_forward(model, batch)
    logits, glogits = result["per_point_logits"], result["global_logits"]
    gt, ggt = batch.y, batch.nocs_grip_point
    weights = (model.nocs_loss_weight, model.grip_point_loss_weight)
    if model.nocs_bins is None:
        mirror = model.symmetry_axis is not None
        return A.value_loss([(logits, gt, "l2", mirror), (glogits, ggt, "l2", mirror)], weights)
    return A.nocs_bin_loss([(logits, gt), (glogits, ggt)], model.nocs_bins, model.symmetry_axis, weights)


def metrics_from_sums(model, sums, result, batch):
    """validation_metrics' five values (python floats) from the loss kernel's sums; the regression head's error distances need the row norms,
    one more launch of gn_value_losses on the detached logits"""
    n, b = batch.y.shape[0], batch.nocs_grip_point.shape[0]
    dist = None
    if model.nocs_bins is None:
        with torch.no_grad():
            d = ops.value_losses([(result["per_point_logits"].detach(), batch.y, "row_norm"),
                                  (result["global_logits"].detach(), batch.nocs_grip_point, "row_norm")]).cpu().tolist()
        dist = (d[0][0], d[1][0])
    return model.metrics_from_sums(sums.cpu().tolist(), n, b, dist)


STAGE = L.Stage(forward=pointnet2_nocs_forward, loss_and_sums=loss_and_sums, metrics_from_sums=metrics_from_sums, metric_keys=lambda model: METRIC_KEYS,
                task_space=False, timing=("seconds",), extras=lambda model: {})
training_step = functools.partial(L.training_step, STAGE)       # (model, batch, batch_idx=None)
training_metrics = functools.partial(L.training_metrics, STAGE)  # (model, batch)
train_step = functools.partial(L.train_step, STAGE)             # (model, optimizer, batch, monitor=None, reducer=None)


# ------------------------------------------------------------------------------------------------ command line
def build_parser():
    ap = validate.build_parser()
    ap.description = "GarmentNets first-stage training (MI355X-native): PointNet2NOCS with FusedAdam over the train subset of a dataset store"
    ap.prog = "python -m garmentnets_amd.train"
    ap.set_defaults(batch_size=8, subset="train")
    L.add_arguments(ap)
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = L.check_arguments(ap, ap.parse_args(argv))
    if a.model == "pipeline":
        raise SystemExit("not implemented yet: second-stage training step")
    return a


def main(argv=None):
    a = parse_args(argv)
    ranks = L.start(a)
    return L.run(STAGE, validate.load_model(a, ranks.device).requires_grad_(True).train(), a, ranks)


if __name__ == "__main__":
    L.command(main)
