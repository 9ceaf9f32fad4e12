"""The first stage's training step: PointNet2NOCS, its loss and Adam, as train_pointnet2.py runs them -- without Hydra, wandb or Lightning.

  pointnet2_nocs_forward(model, data)   PointNet2NOCS.forward's contract and result keys, composed of the differentiable operators of autograd.py
                                        (fps / ball_table / point_conv_max / global_max_pool / knn_interpolate / mlp / linear).  It honours every
                                        module's .training (a stack holding a training BatchNorm normalises with the batch's statistics and updates its
                                        buffers; an eval one folds the running statistics) and the SA modules' random_start, add_self_loops,
                                        self_loop_scope and max_num_neighbors.  A module that needs no gradient and holds no training BatchNorm runs
                                        its own inference forward: with the model in eval mode and under no_grad the result is forward's, bit for bit.
  training_step / training_metrics      the reference's metrics['loss'] as a device scalar with a graph (autograd.nocs_bin_loss over the per-point and the
                                        global row set; autograd.value_loss with l2 in regression mode), and the five logged values from the same sums.
  train_step(model, optimizer, batch)   zero_grad -> training_step -> backward -> optimizer.step()
  python -m garmentnets_amd.train       epochs over the train subset of a dataset store, validate.py's loop on val after each, a csv and a checkpoint;
                                        with --vis_per_items > 0 the reference's monitor images of the selected garments (visualize.py) as PNGs under
                                        <output_dir>/vis/epoch_<NNN>/, rendered from the step's own forward

Real edges only.  Inside the two SA modules local_nn runs over the rows of real edges (slot_src >= 0) and not over the empty slots of the ball table:
BatchNorm statistics and the running buffers see exactly PyG's edge set, which is also what the fused inference kernel later applies them to.

Dropout is the one deliberate exception to "all arithmetic in HIP": the reference's four dropouts (dp1, dp2, global_dp1, global_dp2; p = 0.5, present
iff dropout=True) are torch.nn.functional.dropout on four small tensors, at the reference's positions, when the model is in training mode -- torch's
generator stream could not be matched by a kernel of ours anyway.

Several GPUs: `python -m torch.distributed.run --nproc-per-node N -m garmentnets_amd.train ...` trains data-parallel (parallel.py): every
rank takes its fixed share of the train subset (--batch_size is per rank), train_step gets a GradientReducer, rank 0 alone prints and writes.  Without
torchrun nothing of that runs.

The second stage's step (ConvImplicitWNFPipeline behind this model, frozen) is a module of its own, garmentnets_amd/train_pipeline.py, named after the
reference's script: `python -m garmentnets_amd.train_pipeline`.  It shares _bn_training / _plain / _mlp and _validate with this file; `--model pipeline`
here keeps its refusal.

What stays out: a HIP dropout, a compacting gather kernel in place of the index_select / index_copy
around local_nn.
"""
import argparse
import csv
import json
import os
import time

import torch
import torch.nn.functional as F

from . import autograd as A
from . import ops
from .components.mlp import MLPStack
from .components.pointnet2 import Segments

METRIC_KEYS = ("loss", "nocs_loss", "grip_point_loss", "nocs_err_dist", "grip_point_err_dist")


# ------------------------------------------------------------------------------------------------ the differentiable forward
def _bn_training(stack):
    return any(len(block) > 2 and block[2].training for block in stack)


def _plain(stack, *inputs):
    """True when `stack` can run as its inference forward: no gradient is wanted and no BatchNorm of it is in training mode"""
    if _bn_training(stack):
        return False
    if not torch.is_grad_enabled():
        return True
    return not (any(t is not None and t.requires_grad for t in inputs) or any(p.requires_grad for p in stack.parameters()))


def _mlp(stack, h):
    if not isinstance(stack, MLPStack):
        raise TypeError(f"pointnet2_nocs_forward: expected a components.mlp.MLPStack, got {type(stack).__name__}")
    return A.mlp(stack, h, batch_stats=_bn_training(stack))


def _sa(module, x, pos, seg):
    nn_ = module.conv.local_nn
    if _plain(nn_, x):
        with torch.no_grad():
            return module(x, pos, seg)
    idx = A.fps(pos, seg, module.ratio, random_start=module.random_start)
    cseg = Segments([ops.fps_count(n, module.ratio) for n in seg.sizes], pos.device)
    nbr, _ = A.ball_table(pos, idx, module.r, seg, cseg, module.max_num_neighbors)
    out = A.point_conv_max(x, pos, idx, nbr, lambda e: _mlp(nn_, e), add_self_loops=module.conv.add_self_loops,
                           self_loop_scope=module.conv.self_loop_scope, batch=seg, batch_centre=cseg, real_edges=True)
    return out, pos[idx], cseg


def _global_sa(module, x, pos, seg):
    if _plain(module.nn, x):
        with torch.no_grad():
            return module(x, pos, seg)
    out = A.global_max_pool(_mlp(module.nn, torch.cat((x, pos), 1)), seg)
    return out, pos.new_zeros((seg.num, 3)), Segments([1] * seg.num, pos.device)


def _fp(module, x, pos, seg, x_skip, pos_skip, seg_skip):
    if _plain(module.nn, x, x_skip):
        with torch.no_grad():
            return module(x, pos, seg, x_skip, pos_skip, seg_skip)
    h = A.knn_interpolate(x, pos, pos_skip, seg, seg_skip, k=module.k)
    if x_skip is not None:
        h = torch.cat((h, x_skip), 1)
    return _mlp(module.nn, h), pos_skip, seg_skip


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


def training_step(model, batch, batch_idx=None):
    return loss_and_sums(model, batch)[0]


def training_metrics(model, batch):
    result = pointnet2_nocs_forward(model, batch)
    return metrics_from_sums(model, loss_and_sums(model, batch, result)[1], result, batch)


def train_step(model, optimizer, batch, monitor=None, reducer=None):
    """one optimisation step; -> the detached metrics of the batch (python floats), from the sums of the step's own forward.  monitor: called with
    that forward's result after the step (the training monitors: no second forward).  reducer: a parallel.GradientReducer over `optimizer`
    (data-parallel training): the gradients become their mean over the ranks before the update; None: this process's own, no launch added"""
    optimizer.zero_grad(set_to_none=True)
    result = pointnet2_nocs_forward(model, batch)
    loss, sums = loss_and_sums(model, batch, result)
    loss.backward()
    if reducer is not None:
        reducer.reduce()
    optimizer.step()
    if monitor is not None:
        monitor(result)
    return metrics_from_sums(model, sums, result, batch)


# ------------------------------------------------------------------------------------------------ command line
def build_parser():
    from . import validate
    ap = validate.build_parser()
    ap.description = "GarmentNets first-stage training (MI355X-native): PointNet2NOCS with FusedAdam over the train subset of a dataset store"
    ap.prog = "python -m garmentnets_amd.train"
    ap.set_defaults(batch_size=8, subset="train")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--learning_rate", type=float, default=None, help="default: the model's hyper-parameter")
    ap.add_argument("--seed", type=int, default=0)
    validate.add_resident_arguments(ap)
    validate.add_monitor_arguments(ap)
    return ap


def parse_args(argv=None):
    a = build_parser().parse_args(argv)
    if a.model == "pipeline":
        raise SystemExit("not implemented yet: second-stage training step")
    return a


def _val_dataset(a, volume_task_space=False):
    """the val subset's host dataset: read with static_epoch_seed=True, as the reference's val_dataset"""
    from . import validate
    va = argparse.Namespace(**vars(a))
    va.subset, va.static_epoch_seed = "val", True
    return validate.make_dataset(va, volume_task_space=volume_task_space)


def _validate(model, a, device, volume_task_space=False, resident=None, hook=None, ranks=None):
    """validate.py's loop over the val subset, the model in eval mode for it.  resident: the val subset as a ResidentDataset (built once by the caller);
    None: a host dataset made here.  hook: validation_rows' (the validation monitors).  ranks: parallel.training_ranks' namespace of a data-parallel
    run: this rank loops over its share of the subset (no collective inside the loop) and the garment-weighted means are formed over every rank's sums"""
    from . import parallel, validate
    dataset = _val_dataset(a, volume_task_space) if resident is None else resident.dataset
    indices = dataset.subset_indices("val")
    if ranks is not None and ranks.world > 1:
        indices = parallel.shard_indices(indices, ranks.rank, ranks.world, pad=False)        # (its fixed share, not padded: a partition of the subset)
    was_training = model.training
    model.eval()
    many = ranks is not None and ranks.world > 1
    own = parallel.borrow_buffers(model) if many else None  # (rank 0's running statistics on every rank: the ones last.ckpt holds)
    try:
        rows = validate.validation_rows(model, dataset, indices, a.batch_size, a.num_batches, device,
                                        batches=None if resident is None else resident.batches(indices, a.batch_size), hook=hook)
    finally:
        if many:
            parallel.restore_buffers(model, own)
        model.train(was_training)
    if many:
        return parallel.gather_epoch_values(rows, ranks.metrics_device)
    return validate.epoch_values(rows)


def _data_parallel(model, optimizer, dataset, a, ranks, volume_task_space=False):
    """the data-parallel part of a training loop's set-up -> (reducer, train indices, train resident, val resident).  One process: no reducer, the whole
    subsets.  WORLD_SIZE > 1: rank 0's parameters and buffers everywhere, a GradientReducer, and this rank's fixed shares of the train subset (padded:
    every rank takes the same number of steps) and of the val subset (not padded)"""
    from . import parallel, validate
    indices = dataset.subset_indices("train")
    many = ranks.world > 1
    reducer = None
    if many:
        parallel.broadcast_module(model)
        reducer = parallel.GradientReducer(optimizer, ranks.backend, names=model)
        indices = parallel.shard_indices(indices, ranks.rank, ranks.world, pad=True)
    resident = val_resident = None
    if a.resident:
        tag = ranks.rank if many else None
        resident = validate.make_resident(a, dataset, "train", ranks.device, indices=indices if many else None, rank=tag)
        val_dataset = _val_dataset(a, volume_task_space)
        val_indices = parallel.shard_indices(val_dataset.subset_indices("val"), ranks.rank, ranks.world, pad=False) if many else None
        val_resident = validate.make_resident(a, val_dataset, "val", ranks.device, indices=val_indices, rank=tag)
    return reducer, indices, resident, val_resident


def _train_monitor(writer, batch_idx, batch):
    """train_step's monitor for one batch, from an epoch's visualize.epoch_writer (None: no monitors)"""
    return None if writer is None else lambda result: writer(batch_idx, batch, result)


def main(argv=None):
    from . import parallel, validate, visualize
    a = parse_args(argv)
    ranks = parallel.training_ranks(a.gpu_id)               # (one process: cuda:<gpu_id>; under torch.distributed.run: LOCAL_RANK's device, data-parallel)
    device, chief = ranks.device, ranks.rank == 0
    torch.cuda.set_device(device)
    torch.manual_seed(a.seed + ranks.rank)                  # (the dropout masks differ between the ranks; the data draws are seeded by dataset index)
    model = validate.load_model(a, device).requires_grad_(True).train()
    if a.learning_rate is not None:
        model.learning_rate = model.hparams["learning_rate"] = a.learning_rate
    validate.apply_monitor_arguments(model, a)
    optimizer = model.configure_optimizers()
    a.subset = "train"                                      # (--static_epoch_seed: the same draws every epoch, for a reproducible run)
    dataset = validate.make_dataset(a)
    reducer, indices, resident, val_resident = _data_parallel(model, optimizer, dataset, a, ranks)
    if chief:
        os.makedirs(os.path.join(a.output_dir, "checkpoints"), exist_ok=True)
    rows, epochs = [], []
    for epoch in range(a.epochs):
        order = validate.epoch_order(indices, a.shuffle, a.seed, epoch)
        source = resident.batches(order, a.batch_size) if a.resident else validate.host_batches(dataset, order, a.batch_size)
        writer = visualize.epoch_writer(model, a.output_dir, epoch, True) if chief else None
        for batch_idx, (chunk, batch) in enumerate(source):
            if a.num_batches is not None and batch_idx >= a.num_batches:
                break
            t0 = time.time()
            batch = batch.to(device)
            metrics = train_step(model, optimizer, batch, _train_monitor(writer, batch_idx, batch), reducer=reducer)
            row = {"epoch": epoch, "batch_idx": batch_idx, "garments": len(chunk), "seconds": time.time() - t0}
            if ranks.world > 1:
                row["world"] = ranks.world
            if a.resident:
                row["resident"] = True
            row.update({"train_" + k: float(v) for k, v in metrics.items()})
            rows.append(row)
            if chief:
                print(json.dumps(row))
        val = _validate(model, a, device, resident=val_resident, hook=visualize.epoch_writer(model, a.output_dir, epoch, False) if chief else None,
                        ranks=ranks)
        epochs.append(dict(epoch=epoch, **val))
        if chief:
            print(json.dumps(epochs[-1]))
            torch.save({"state_dict": model.state_dict(), "hyper_parameters": model.hparams, "optimizer_states": [optimizer.state_dict()],
                        "epoch": epoch}, os.path.join(a.output_dir, "checkpoints", "last.ckpt"))
    result = {"model": model, "optimizer": optimizer, "train_rows": rows, "val_epochs": epochs, "resident": resident, "val_resident": val_resident}
    if not chief:                                           # (rank 0 alone writes: the csv holds its own batches' metrics, the checkpoint its buffers)
        return result
    cols = ["epoch", "batch_idx", "garments", "seconds"] + (["world"] if ranks.world > 1 else []) + (["resident"] if a.resident else []) + ["train_" + k for k in METRIC_KEYS]
    with open(os.path.join(a.output_dir, "train_metrics.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=cols)
        w.writeheader()
        for r in rows:
            w.writerow({k: r.get(k, "") for k in cols})
    with open(os.path.join(a.output_dir, "val_epochs.json"), "w") as f:
        json.dump(epochs, f, indent=2)
    return result


if __name__ == "__main__":
    main()
    from . import parallel
    parallel.finish()
