"""The training loop both stages run: one step, one command line's worth of shared flags, one epoch loop with its validation, checkpoint and outputs.

A stage (train.py: PointNet2NOCS; train_pipeline.py: ConvImplicitWNFPipeline behind it) describes itself in a Stage record and keeps its differentiable
forward, its loss, its own flags and its model's set-up.  Nothing here asks which stage it serves: it reads the record.

  bn_training / plain / mlp             the rule every differentiable forward follows for an MLPStack: a stack holding a training BatchNorm normalises
                                        with the batch's statistics; one that needs no gradient and holds none runs its inference forward
  train_step(stage, model, optimizer, batch, monitor, reducer)
                                        zero_grad -> forward -> loss -> backward -> reducer.reduce() -> optimizer.step() -> monitor(result), then the
                                        metrics from the sums of that one forward; nothing is read back between forward and backward
  training_step / training_metrics      the loss with its graph, and the logged values, of one batch
  add_arguments(ap)                     --epochs, --learning_rate, --seed, the data-source flags (--resident, --resident_gib, --exact_targets, --shuffle) and the monitor
                                        flags (--vis_per_items, --max_vis_per_epoch_train, --max_vis_per_epoch_val)
  start(a)                              parallel.training_ranks, the device, torch.manual_seed(seed + rank): what precedes the model's construction
  run(stage, model, a, ranks)           the learning-rate override, the monitor arguments, the optimizer, the train dataset, the data-parallel set-up;
                                        then per epoch the steps over the train subset (one printed row each), validate.py's loop on val, an epoch
                                        record and checkpoints/last.ckpt; at the end train_metrics.csv and val_epochs.json
  command(main)                         a stage's `python -m` entry: main(), then parallel.finish()

Several GPUs: `python -m torch.distributed.run --nproc-per-node N -m garmentnets_amd.train ...` (or .train_pipeline) trains data-parallel (parallel.py,
DESIGN.md 6): every rank takes its fixed share of the train subset (--batch_size is per rank), train_step gets a GradientReducer, validation borrows
rank 0's buffers and restores them, rank 0 alone prints and writes.  Without torchrun nothing of that runs.

--num_batches is looked at before a batch is fetched: none is assembled and thrown away.  A row's "seconds" runs from after the fetch to after the step,
its "data_seconds" (a stage that lists it) is the host time of the fetch.
"""
import argparse
import csv
import json
import os
import time
from typing import Callable, NamedTuple, Tuple

import numpy as np
import torch

from . import autograd as A
from . import parallel, validate, visualize
from .components.mlp import MLPStack


class Stage(NamedTuple):
    """what the loop has to know about a stage"""
    forward: Callable                   # (model, batch) -> the result dict of the model's forward, differentiable
    loss_and_sums: Callable             # (model, batch, result) -> (loss with its graph, the detached sums of the loss kernel)
    metrics_from_sums: Callable         # (model, sums, result, batch) -> {metric: python float}
    metric_keys: Callable               # (model) -> the metrics' names, in the csv's column order
    task_space: bool                    # the datasets take volume_task_space from the model
    timing: Tuple[str, ...]             # a row's timing columns, of "data_seconds" (fetching the batch) and "seconds" (the step)
    extras: Callable                    # (model) -> the further entries of a printed row and of an epoch record (not of the csv)


# ------------------------------------------------------------------------------------------------ the differentiable forwards' shared rule
def bn_training(stack):
    return any(len(block) > 2 and block[2].training for block in stack)


def plain(stack, *inputs):
    """True when `stack` can run as its inference forward: no gradient is wanted and no BatchNorm of it is in training mode"""
    if bn_training(stack):
        return False
    if not torch.is_grad_enabled():
        return True
    return not (any(t is not None and t.requires_grad for t in inputs) or any(p.requires_grad for p in stack.parameters()))


def mlp(stack, h):
    if not isinstance(stack, MLPStack):
        raise TypeError(f"pointnet2_nocs_forward: expected a components.mlp.MLPStack, got {type(stack).__name__}")
    return A.mlp(stack, h, batch_stats=bn_training(stack))


# ------------------------------------------------------------------------------------------------ the step
def training_step(stage, model, batch, batch_idx=None):
    return stage.loss_and_sums(model, batch, stage.forward(model, batch))[0]


def training_metrics(stage, model, batch):
    result = stage.forward(model, batch)
    return stage.metrics_from_sums(model, stage.loss_and_sums(model, batch, result)[1], result, batch)


def train_step(stage, model, optimizer, batch, monitor=None, reducer=None):
    """one optimisation step; -> the detached metrics of the batch (python floats), from the sums of the step's own forward.  monitor: called with
    that forward's result after the step (the training monitors: no second forward).  reducer: a parallel.GradientReducer over `optimizer`
    (data-parallel training): the gradients become their mean over the ranks before the update; None: this process's own, no launch added"""
    optimizer.zero_grad(set_to_none=True)
    result = stage.forward(model, batch)
    loss, sums = stage.loss_and_sums(model, batch, result)
    loss.backward()
    if reducer is not None:
        reducer.reduce()
    optimizer.step()
    if monitor is not None:
        monitor(result)
    return stage.metrics_from_sums(model, sums, result, batch)


# ------------------------------------------------------------------------------------------------ command line
def add_arguments(ap):
    """the flags of both training command lines, on top of validate.build_parser's"""
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--learning_rate", type=float, default=None, help="default: the model's hyper-parameter")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--resident", action="store_true",
                    help="read the train and the val subset once into device memory (io/resident.py) and assemble every batch there")
    ap.add_argument("--resident_gib", type=float, default=None, help="device-memory budget of EACH resident subset; default: half of what is free")
    ap.add_argument("--exact_targets", action="store_true", default=argparse.SUPPRESS,      # (absent from the namespace unless given: exact_targets(a))
                    help="with --resident: take gt_volume_value from the garment's own mesh at the query points (targets.py) instead of a stored volume; "
                         "the store then needs no `volume` group")
    ap.add_argument("--shuffle", action="store_true",
                    help="visit the train subset in a RandomState(seed + epoch) permutation (the reference's train_dataloader: shuffle=True)")
    # the reference's three hyper-parameters of vis_batch
    ap.add_argument("--vis_per_items", type=int, default=None,
                    help="draw every this-many-th garment of an epoch into <output_dir>/vis/epoch_<NNN>/ (0: none); default: the model's hyper-parameter")
    ap.add_argument("--max_vis_per_epoch_train", type=int, default=None, help="at most this many train images per epoch; default: the model's")
    ap.add_argument("--max_vis_per_epoch_val", type=int, default=None, help="at most this many val images per epoch; default: the model's")


def exact_targets(a):
    """--exact_targets of a parsed namespace"""
    return bool(getattr(a, "exact_targets", False))


def check_arguments(ap, a):
    """what the flags of add_arguments owe each other, as an argparse error of `ap`"""
    if exact_targets(a) and not a.resident:
        ap.error("--exact_targets requires --resident: the exact targets are built on the device from the resident meshes")
    return a


def apply_monitor_arguments(model, a):
    """the three flags that were given replace the model's hyper-parameters (and travel in its checkpoints); the model learns the loop's batch size,
    which get_vis_idxs numbers the garments of an epoch with"""
    for key in ("vis_per_items", "max_vis_per_epoch_train", "max_vis_per_epoch_val"):
        if getattr(a, key) is not None:
            setattr(model, key, getattr(a, key))
            model.hparams[key] = getattr(a, key)
    model.batch_size = a.batch_size


def epoch_order(indices, shuffle, seed, epoch):
    """the order of the train subset in `epoch`"""
    indices = np.asarray(indices)
    return indices[np.random.RandomState(seed + epoch).permutation(len(indices))] if shuffle else indices


def make_resident(a, dataset, subset, device, indices=None, rank=None):
    """the subset of `dataset` as a ResidentDataset under --resident_gib; prints its one-off load time and footprint.  indices: this rank's share of
    the subset (parallel.shard_indices) in place of all of it; the report of EVERY rank then carries its rank and its index list"""
    from .io.resident import ResidentDataset
    budget = None if a.resident_gib is None else int(a.resident_gib * 2 ** 30)
    exact = exact_targets(a)
    res = ResidentDataset(dataset, dataset.subset_indices(subset) if indices is None else indices, device, max_bytes=budget, exact_targets=exact)
    report = {"resident_subset": subset, "samples": len(res), "nbytes": res.nbytes, "load_seconds": res.load_seconds}
    if exact:
        report["exact_targets"] = res.exact_targets
    if rank is not None:
        report.update(rank=rank, indices=res.indices)
    print(json.dumps(report), flush=rank is not None)
    return res


# ------------------------------------------------------------------------------------------------ validation, data parallelism, monitors
def _val_dataset(a, volume_task_space=False):
    """the val subset's host dataset: read with static_epoch_seed=True, as the reference's val_dataset"""
    va = argparse.Namespace(**vars(a))
    va.subset, va.static_epoch_seed = "val", True
    return validate.make_dataset(va, volume_task_space=volume_task_space)


def _validate(model, a, device, volume_task_space=False, resident=None, hook=None, ranks=None):
    """validate.py's loop over the val subset, the model in eval mode for it.  resident: the val subset as a ResidentDataset (built once by the caller);
    None: a host dataset made here.  hook: validation_rows' (the validation monitors).  ranks: parallel.training_ranks' namespace of a data-parallel
    run: this rank loops over its share of the subset (no collective inside the loop) and the garment-weighted means are formed over every rank's sums"""
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
    """the data-parallel part of the set-up -> (reducer, train indices, train resident, val resident).  One process: no reducer, the whole subsets.
    WORLD_SIZE > 1: rank 0's parameters and buffers everywhere, a GradientReducer, and this rank's fixed shares of the train subset (padded: every
    rank takes the same number of steps) and of the val subset (not padded)"""
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
        resident = make_resident(a, dataset, "train", ranks.device, indices=indices if many else None, rank=tag)
        val_dataset = _val_dataset(a, volume_task_space)
        val_indices = parallel.shard_indices(val_dataset.subset_indices("val"), ranks.rank, ranks.world, pad=False) if many else None
        val_resident = make_resident(a, val_dataset, "val", ranks.device, indices=val_indices, rank=tag)
    return reducer, indices, resident, val_resident


def _train_monitor(writer, batch_idx, batch):
    """train_step's monitor for one batch, from an epoch's visualize.epoch_writer (None: no monitors)"""
    return None if writer is None else lambda result: writer(batch_idx, batch, result)


# ------------------------------------------------------------------------------------------------ rows, columns, the loop
def _flags(world, resident, exact_targets=False):
    """a row's entries that only a data-parallel, only a --resident and only an --exact_targets run have"""
    return {**({"world": world} if world > 1 else {}), **({"resident": True} if resident else {}), **({"exact_targets": True} if exact_targets else {})}


def train_row(stage, model, epoch, batch_idx, garments, seconds, world, resident, metrics, exact_targets=False):
    """the printed row of one step, in its key order.  seconds: {"data_seconds": .., "seconds": ..}, of which the stage's timing columns are kept"""
    return {"epoch": epoch, "batch_idx": batch_idx, "garments": garments, **{k: seconds[k] for k in stage.timing}, **stage.extras(model),
            **_flags(world, resident, exact_targets), **{"train_" + k: float(v) for k, v in metrics.items()}}


def csv_columns(stage, model, world, resident, exact_targets=False):
    """train_metrics.csv's columns: a row's keys without the stage's extras"""
    return ["epoch", "batch_idx", "garments", *stage.timing, *_flags(world, resident, exact_targets), *("train_" + k for k in stage.metric_keys(model))]


def _write_outputs(output_dir, cols, rows, epochs):
    with open(os.path.join(output_dir, "train_metrics.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=cols)
        w.writeheader()
        for r in rows:
            w.writerow({k: r.get(k, "") for k in cols})
    with open(os.path.join(output_dir, "val_epochs.json"), "w") as f:
        json.dump(epochs, f, indent=2)


def start(a):
    """-> parallel.training_ranks' namespace; this process's device is made current and torch is seeded with --seed + rank"""
    ranks = parallel.training_ranks(a.gpu_id)               # (one process: cuda:<gpu_id>; under torch.distributed.run: LOCAL_RANK's device, data-parallel)
    torch.cuda.set_device(ranks.device)
    torch.manual_seed(a.seed + ranks.rank)                  # (the dropout masks differ between the ranks; the data draws are seeded by dataset index)
    return ranks


def run(stage, model, a, ranks):
    """train `model` (on ranks.device, in training mode, its arithmetic set) as the arguments `a` say -> the model, the optimizer, the rows, the epoch
    records and the resident datasets"""
    device, chief = ranks.device, ranks.rank == 0
    if a.learning_rate is not None:
        model.learning_rate = model.hparams["learning_rate"] = a.learning_rate
    apply_monitor_arguments(model, a)
    optimizer = model.configure_optimizers()
    a.subset = "train"                                      # (--static_epoch_seed: the same draws every epoch, for a reproducible run)
    task = model.volume_task_space if stage.task_space else False
    dataset = validate.make_dataset(a, volume_task_space=task)
    reducer, indices, resident, val_resident = _data_parallel(model, optimizer, dataset, a, ranks, volume_task_space=task)
    exact = resident is not None and resident.exact_targets  # (--exact_targets where the stage samples volume queries at all)
    if chief:
        os.makedirs(os.path.join(a.output_dir, "checkpoints"), exist_ok=True)
    rows, epochs = [], []
    for epoch in range(a.epochs):
        order = epoch_order(indices, a.shuffle, a.seed, epoch)
        batches = resident.batches(order, a.batch_size) if a.resident else validate.host_batches(dataset, order, a.batch_size)
        writer = visualize.epoch_writer(model, a.output_dir, epoch, True) if chief else None
        batch_idx = 0
        while a.num_batches is None or batch_idx < a.num_batches:
            t0 = time.time()
            item = next(batches, None)                      # host: read, sample and collate one batch; resident: draw, upload, launch
            if item is None:
                break
            chunk, batch = item
            t1 = time.time()
            batch = batch.to(device)
            metrics = train_step(stage, model, optimizer, batch, _train_monitor(writer, batch_idx, batch), reducer=reducer)
            seconds = {"data_seconds": t1 - t0, "seconds": time.time() - t1}
            rows.append(train_row(stage, model, epoch, batch_idx, len(chunk), seconds, ranks.world, a.resident, metrics, exact))
            if chief:
                print(json.dumps(rows[-1]))
            batch_idx += 1
        val = _validate(model, a, device, volume_task_space=task, resident=val_resident,
                        hook=visualize.epoch_writer(model, a.output_dir, epoch, False) if chief else None, ranks=ranks)
        epochs.append({"epoch": epoch, **stage.extras(model), **val})
        if chief:
            print(json.dumps(epochs[-1]))
            torch.save({"state_dict": model.state_dict(), "hyper_parameters": model.hparams, "optimizer_states": [optimizer.state_dict()],
                        "epoch": epoch}, os.path.join(a.output_dir, "checkpoints", "last.ckpt"))
    if chief:                                               # (rank 0 alone writes: the csv holds its own batches' metrics, the checkpoint its buffers)
        _write_outputs(a.output_dir, csv_columns(stage, model, ranks.world, a.resident, exact), rows, epochs)
    return {"model": model, "optimizer": optimizer, "train_rows": rows, "val_epochs": epochs, "resident": resident, "val_resident": val_resident}


def command(main):
    main()
    parallel.finish()
