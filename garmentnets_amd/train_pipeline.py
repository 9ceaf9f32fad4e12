"""The second stage's training step: ConvImplicitWNFPipeline behind a frozen PointNet2NOCS, its weighted loss and Adam, as train_pipeline.py runs them
-- without Hydra, wandb or Lightning.

  pipeline_forward(model, data, arith)  ConvImplicitWNFPipeline.forward's contract and result keys, differentiable in every parameter of volume_agg, unet_3d
                                        and the two or three decoders: autograd.mlp -> autograd.scatter -> autograd.unet3d -> autograd.implicit_decode per
                                        head on the one volume (the engine's add is where the heads' volume gradients meet).  Every MLPStack honours its own
                                        .training (train.py's rule).  When no gradient is wanted and no BatchNorm of the second stage is in training mode it
                                        IS model.forward(data, arith): the fused decoders, the occupancy-aware first convolution, forward's bits.
  training_step / training_metrics      the reference's metrics['loss'] as a device scalar with a graph (ONE autograd.value_loss over the segments
                                        ConvImplicitWNFPipeline.loss_segments forms, which validation reads too), and the logged values from the same sums.
  train_step(model, optimizer, batch)   zero_grad -> forward -> backward -> optimizer.step(); nothing is read back between forward and backward
  python -m garmentnets_amd.train_pipeline
                                        epochs over the train subset of a dataset store, validate.py's loop on val after each, a csv and a checkpoint.
                                        It trains with arith.device_packs: the UNet's static weight packs, stale after every optimiser step, are rebuilt
                                        on the device (csrc/weight_pack.hip; same bits) instead of through the host; --host_packs keeps the host builders.
                                        --split_backward: the UNet convolutions' gradients on the 16-bit matrix cores (arith.conv_grad_mode = "f16x2",
                                        csrc/unet_grad_split.hip); without it the backward is fp32, today's launches.
                                        --vis_per_items > 0: the reference's monitor images of the selected garments (visualize.py) as PNGs under
                                        <output_dir>/vis/epoch_<NNN>/, rendered from the step's own forward

The first stage is frozen, as the reference's pointnet2_forward freezes it on every call: pointnet2_nocs is put in eval mode (and left there, whatever
model.train() said before) and runs its inference forward under no_grad.  None of its parameters or buffers changes and none gets a .grad; they stay in
configure_optimizers' one group, where FusedAdam skips a parameter without a gradient.  ops.grid_features (the rows the aggregator reads and the cell of
every point) is data: no gradient reaches the predicted NOCS coordinates or the confidences.

The stages are functions of their own (first_stage / aggregate / unet / heads) so that tools/pipeline_step_time.py can bracket them and the tests can
record the second stage alone.

--resident holds the train and the val subset in device memory and assembles every batch there (io/resident.py); each csv row records data_seconds, the
host time until the batch is handed to the step, either way.

Several GPUs: `python -m torch.distributed.run --nproc-per-node N -m garmentnets_amd.train_pipeline ...` trains data-parallel, as train.py does (its
docstring; parallel.py): the frozen first stage has no gradient and stays out of the reduced buffer; BatchNorm running buffers stay per rank.

What stays out: a worker pool for the host dataset, a backward for the fused inference kernels, SyncBN, overlap of the all-reduce with the backward.
"""
import csv
import json
import os
import time

import torch

from . import autograd as A
from . import ops
from .train import _bn_training, _data_parallel, _mlp, _plain, _train_monitor, _validate

HEADS = (("volume_decoder", "volume_decoder_result", "volume_query_points"), ("surface_decoder", "surface_decoder_result", "surf_query_points"),
         ("mc_surface_decoder", "mc_surface_decoder_result", "mc_surf_query_points"))


# ------------------------------------------------------------------------------------------------ the differentiable forward
def second_stage_stacks(model):
    """the MLPStacks of the second stage: the aggregator's and every decoder's"""
    stacks = [] if model.volume_agg.local_nn is None else [model.volume_agg.local_nn]
    return stacks + [getattr(model, name).mlp for name, _, _ in HEADS if getattr(model, name, None) is not None]


def _inference(model):
    """True when pipeline_forward is model.forward itself: no gradient is wanted and no BatchNorm of the second stage is in training mode"""
    if torch.is_grad_enabled() and any(p.requires_grad for p in model.unet_3d.parameters()):
        return False
    return all(_plain(stack) for stack in second_stage_stacks(model))


def first_stage(model, data):
    """-> pointnet2_result: model.pointnet2_forward as it is, under no_grad, pointnet2_nocs in eval mode; in task space when the model says so"""
    model.pointnet2_nocs.eval()
    with torch.no_grad():
        p2 = model.pointnet2_forward(data)
        if model.volume_task_space:
            p2 = model.apply_volume_task_space(data, p2)
    return p2


def aggregate(model, nocs_data):
    """VolumeFeatureAggregator.forward's contract -> (B, C, G, G, G), a view over channel-last storage, differentiable in local_nn's parameters"""
    agg = model.volume_agg
    if agg.reduce_method == "mul" and torch.is_grad_enabled() and agg.local_nn is not None and any(p.requires_grad for p in agg.local_nn.parameters()):
        raise ValueError("pipeline_forward: reduce_method='mul' has no gradient here (autograd.scatter refuses it: nobody trains with it)")
    with torch.no_grad():
        feats, flat = ops.grid_features(nocs_data.x, nocs_data.pos.contiguous(), nocs_data.sim_points.float().contiguous(),
                                        nocs_data.pred_confidence.contiguous(), nocs_data.batch, agg.lower_corner, agg.upper_corner, agg.grid_shape,
                                        agg.include_point_feature, agg.include_confidence_feature)
    if agg.local_nn is not None:
        feats = _mlp(agg.local_nn, feats)
    B, C = nocs_data.num_graphs, feats.shape[1]
    cells = B * agg.grid_shape[0] * agg.grid_shape[1] * agg.grid_shape[2]
    vol = A.scatter(feats.t(), flat, -1, cells, agg.reduce_method)
    return vol.view(C, B, *agg.grid_shape).permute(1, 0, 2, 3, 4)


def unet(model, volume, arith=None):
    """-> the unet3d_result dict; the forward arithmetic is `arith` (None: the model's), the backward fp32 (autograd.unet3d)"""
    return {"out_feature_volume": A.unet3d(model.unet_3d.abstract_3d_unet, volume, arith or model.arith)}


def heads(model, unet3d_result, data):
    """every decoder on the one volume -> the decoder result dicts of forward, by their keys"""
    vol = unet3d_result["out_feature_volume"]
    out = {}
    for name, key, queries in HEADS:
        decoder = getattr(model, name, None)
        if decoder is None:
            continue
        y = A.implicit_decode(decoder, vol, getattr(data, queries), batch_stats=_bn_training(decoder.mlp))
        out[key] = {"out_features": y}
        if name == "volume_decoder":
            out[key]["pred_volume_value"] = y.view(*y.shape[:-1])
    return out


def pipeline_forward(model, data, arith=None):
    """ConvImplicitWNFPipeline.forward's contract and result keys, differentiable in every parameter of the second stage (the module docstring)"""
    if _inference(model):
        model.pointnet2_nocs.eval()
        with torch.no_grad():
            return model.forward(data, arith)
    p2 = first_stage(model, data)
    u3 = unet(model, aggregate(model, p2["nocs_data"]), arith)
    return {"pointnet2_result": p2, "unet3d_result": u3, **heads(model, u3, data)}


# ------------------------------------------------------------------------------------------------ loss, metrics, step
def loss_and_sums(model, batch, result=None):
    """-> (loss, sums): the reference's loss of one batch as a device scalar with a graph, and the detached (segments, 2) fp64 sums of the loss kernel
    (the metrics are formed from them: no second forward).  One launch over the segments of ConvImplicitWNFPipeline.loss_segments"""
    if result is None:
        result = pipeline_forward(model, batch)
    segs, _, weights = model.loss_segments(result, batch)
    return A.value_loss(segs, weights)


def metrics_from_sums(model, sums, result, batch):
    """validation_metrics' values (python floats) from the loss kernel's sums: losses_from's own expression"""
    segs, names, weights = model.loss_segments(result, batch)
    return model.metrics_from_sums(sums[:, 0].cpu().tolist(), names, weights, [seg[1].numel() for seg in segs])


def metric_keys(model):
    return ("loss", "volume_loss", "surface_loss") + (("mc_surface_loss",) if model.mc_surface_loss_weight > 0 else ())


def training_step(model, batch, batch_idx=None):
    return loss_and_sums(model, batch)[0]


def training_metrics(model, batch):
    result = pipeline_forward(model, batch)
    return metrics_from_sums(model, loss_and_sums(model, batch, result)[1], result, batch)


def train_step(model, optimizer, batch, monitor=None, reducer=None):
    """one optimisation step; -> the detached metrics of the batch (python floats), from the sums of the step's own forward.  monitor: called with
    that forward's result after the step (the training monitors: no second forward).  reducer: a parallel.GradientReducer over `optimizer`
    (data-parallel training): the gradients become their mean over the ranks before the update; None: this process's own, no launch added"""
    optimizer.zero_grad(set_to_none=True)
    result = pipeline_forward(model, batch)
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
    ap.description = ("GarmentNets second-stage training (MI355X-native): ConvImplicitWNFPipeline behind a frozen PointNet2NOCS, with FusedAdam over the "
                      "train subset of a dataset store")
    ap.prog = "python -m garmentnets_amd.train_pipeline"
    ap.set_defaults(model="pipeline", batch_size=24, subset="train")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--learning_rate", type=float, default=None, help="default: the model's hyper-parameter")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pointnet2_checkpoint", default=None,
                    help="Lightning-style .ckpt of a PointNet2NOCS: it becomes the model's first stage (and its pointnet2_params)")
    ap.add_argument("--host_packs", action="store_true",
                    help="build the UNet's static weight packs on the host after every step (the inference path's builders) instead of on the device "
                         "(arith.device_packs: same bits, no stream synchronisation)")
    ap.add_argument("--split_backward", action="store_true",
                    help="run the gradients of the UNet's 3x3x3 convolutions on the 16-bit matrix cores (arith.conv_grad_mode = 'f16x2': fp16 operand "
                         "planes, fp32 accumulation); default: the fp32 backward")
    validate.add_resident_arguments(ap)
    validate.add_monitor_arguments(ap)
    return ap


def parse_args(argv=None):
    a = build_parser().parse_args(argv)
    if a.model != "pipeline":
        raise SystemExit("garmentnets_amd.train_pipeline trains the pipeline model; the first stage's step is python -m garmentnets_amd.train")
    return a


def load_model(a, device):
    """the model to train.  --checkpoint_path: that pipeline checkpoint; neither checkpoint: validate.load_model's seeded synthetic weights; only
    --pointnet2_checkpoint: the second-stage modules keep their constructors' initialisation (under torch.manual_seed(--seed)).  A
    --pointnet2_checkpoint replaces the first stage, and hparams["pointnet2_params"], in every case."""
    from . import synthetic, validate
    from .networks.conv_implicit_wnf import ConvImplicitWNFPipeline
    from .networks.pointnet2_nocs import PointNet2NOCS
    if a.checkpoint_path or not a.pointnet2_checkpoint:
        model = validate.load_model(a, device)
    else:
        hp = synthetic.default_hparams(grid=a.grid, reduce_method=a.reduce_method, mc_surface=a.mc_surface)
        model = ConvImplicitWNFPipeline(**hp)
    if a.pointnet2_checkpoint:
        first = PointNet2NOCS.load_from_checkpoint(a.pointnet2_checkpoint)
        model.pointnet2_nocs = first
        model.hparams["pointnet2_params"] = dict(first.hparams)
        model.pointnet2_nocs.set_self_loop_scope(a.self_loop_scope)
    return model.to(device)


def main(argv=None):
    from . import parallel, validate, visualize
    a = parse_args(argv)
    ranks = parallel.training_ranks(a.gpu_id)               # (one process: cuda:<gpu_id>; under torch.distributed.run: LOCAL_RANK's device, data-parallel)
    device, chief = ranks.device, ranks.rank == 0
    torch.cuda.set_device(device)
    torch.manual_seed(a.seed + ranks.rank)
    model = load_model(a, device).requires_grad_(True).train()
    model.arith = model.arith.replace(device_packs=not a.host_packs)        # (train_step reads the model's arithmetic)
    if a.split_backward:
        model.arith = model.arith.replace(conv_grad_mode="f16x2")
    if a.learning_rate is not None:
        model.learning_rate = model.hparams["learning_rate"] = a.learning_rate
    validate.apply_monitor_arguments(model, a)
    optimizer = model.configure_optimizers()
    a.subset = "train"                                      # (--static_epoch_seed: the same draws every epoch, for a reproducible run)
    dataset = validate.make_dataset(a, volume_task_space=model.volume_task_space)
    task = model.volume_task_space
    reducer, indices, resident, val_resident = _data_parallel(model, optimizer, dataset, a, ranks, volume_task_space=task)
    if chief:
        os.makedirs(os.path.join(a.output_dir, "checkpoints"), exist_ok=True)
    keys = metric_keys(model)
    rows, epochs = [], []
    for epoch in range(a.epochs):
        order = validate.epoch_order(indices, a.shuffle, a.seed, epoch)
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
            metrics = train_step(model, optimizer, batch, _train_monitor(writer, batch_idx, batch), reducer=reducer)
            row = {"epoch": epoch, "batch_idx": batch_idx, "garments": len(chunk), "data_seconds": t1 - t0, "seconds": time.time() - t1,
                   "device_packs": model.arith.device_packs}
            if ranks.world > 1:
                row["world"] = ranks.world
            if a.resident:
                row["resident"] = True
            row.update({"train_" + k: float(v) for k, v in metrics.items()})
            rows.append(row)
            if chief:
                print(json.dumps(row))
            batch_idx += 1
        val = _validate(model, a, device, volume_task_space=task, resident=val_resident,
                        hook=visualize.epoch_writer(model, a.output_dir, epoch, False) if chief else None, ranks=ranks)
        epochs.append(dict(epoch=epoch, device_packs=model.arith.device_packs, **val))
        if chief:
            print(json.dumps(epochs[-1]))
            torch.save({"state_dict": model.state_dict(), "hyper_parameters": model.hparams, "optimizer_states": [optimizer.state_dict()],
                        "epoch": epoch}, os.path.join(a.output_dir, "checkpoints", "last.ckpt"))
    result = {"model": model, "optimizer": optimizer, "train_rows": rows, "val_epochs": epochs, "resident": resident, "val_resident": val_resident}
    if not chief:                                           # (rank 0 alone writes: the csv holds its own batches' metrics, the checkpoint its buffers)
        return result
    cols = (["epoch", "batch_idx", "garments", "data_seconds", "seconds"] + (["world"] if ranks.world > 1 else []) + (["resident"] if a.resident else []) +
            ["train_" + k for k in keys])
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
