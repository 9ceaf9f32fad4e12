"""The second stage's training step: ConvImplicitWNFPipeline behind a frozen PointNet2NOCS, its weighted loss and Adam, as train_pipeline.py runs them
-- without Hydra, wandb or Lightning.

  pipeline_forward(model, data, arith)  ConvImplicitWNFPipeline.forward's contract and result keys, differentiable in every parameter of volume_agg, unet_3d
                                        and the two or three decoders: autograd.mlp -> autograd.scatter -> autograd.unet3d -> autograd.implicit_decode per
                                        head on the one volume (the engine's add is where the heads' volume gradients meet).  Every MLPStack honours its own
                                        .training (train_loop.py's rule).  When no gradient is wanted and no BatchNorm of the second stage is in training
                                        mode it IS model.forward(data, arith): the fused decoders, the occupancy-aware first convolution, forward's bits.
  loss_and_sums / metrics_from_sums     the reference's metrics['loss'] as a device scalar with a graph (ONE autograd.value_loss over the segments
                                        ConvImplicitWNFPipeline.loss_segments forms, which validation reads too), and the logged values from the same sums.
  STAGE                                 this stage as train_loop.py's loop reads it; train_step / training_step / training_metrics are the loop's, bound to it
  python -m garmentnets_amd.train_pipeline
                                        train_loop.run over the train subset of a dataset store (train_loop.py's docstring), every row with data_seconds,
                                        the host time until the batch is handed to the step, and with device_packs.
                                        It trains with arith.device_packs: the UNet's static weight packs, stale after every optimiser step, are rebuilt
                                        on the device (csrc/weight_pack.hip; same bits) instead of through the host; --host_packs keeps the host builders.
                                        --split_backward: the UNet convolutions' gradients on the 16-bit matrix cores (arith.conv_grad_mode = "f16x2",
                                        csrc/unet_grad_split.hip); without it the backward is fp32.
                                        --pointnet2_checkpoint: a trained first stage in place of the model's own

The first stage is frozen, as the reference's pointnet2_forward freezes it on every call: pointnet2_nocs is put in eval mode (and left there, whatever
model.train() said before) and runs its inference forward under no_grad.  None of its parameters or buffers changes and none gets a .grad; they stay in
configure_optimizers' one group, where FusedAdam skips a parameter without a gradient.  ops.grid_features (the rows the aggregator reads and the cell of
every point) is data: no gradient reaches the predicted NOCS coordinates or the confidences.

The stages are functions of their own (first_stage / aggregate / unet / heads) so that tools/pipeline_step_time.py can bracket them and the tests can
record the second stage alone.

Several GPUs (train_loop.py's docstring; parallel.py): the frozen first stage has no gradient and stays out of the reduced buffer; BatchNorm running
buffers stay per rank.

What stays out: a worker pool for the host dataset, a backward for the fused inference kernels, SyncBN, overlap of the all-reduce with the backward.
"""
import functools

import torch

from . import autograd as A
from . import ops
from . import train_loop as L
from . import validate

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
    return all(L.plain(stack) for stack in second_stage_stacks(model))


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
        feats = L.mlp(agg.local_nn, feats)
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
        y = A.implicit_decode(decoder, vol, getattr(data, queries), batch_stats=L.bn_training(decoder.mlp))
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


STAGE = L.Stage(forward=pipeline_forward, loss_and_sums=loss_and_sums, metrics_from_sums=metrics_from_sums, metric_keys=metric_keys, task_space=True,
                timing=("data_seconds", "seconds"), extras=lambda model: {"device_packs": model.arith.device_packs})
training_step = functools.partial(L.training_step, STAGE)       # (model, batch, batch_idx=None)
training_metrics = functools.partial(L.training_metrics, STAGE)  # (model, batch)
train_step = functools.partial(L.train_step, STAGE)             # (model, optimizer, batch, monitor=None, reducer=None)


# ------------------------------------------------------------------------------------------------ command line
def build_parser():
    ap = validate.build_parser()
    ap.description = ("GarmentNets second-stage training (MI355X-native): ConvImplicitWNFPipeline behind a frozen PointNet2NOCS, with FusedAdam over the "
                      "train subset of a dataset store")
    ap.prog = "python -m garmentnets_amd.train_pipeline"
    ap.set_defaults(model="pipeline", batch_size=24, subset="train")
    L.add_arguments(ap)
    ap.add_argument("--pointnet2_checkpoint", default=None,
                    help="Lightning-style .ckpt of a PointNet2NOCS: it becomes the model's first stage (and its pointnet2_params)")
    ap.add_argument("--host_packs", action="store_true",
                    help="build the UNet's static weight packs on the host after every step (the inference path's builders) instead of on the device "
                         "(arith.device_packs: same bits, no stream synchronisation)")
    ap.add_argument("--split_backward", action="store_true",
                    help="run the gradients of the UNet's 3x3x3 convolutions on the 16-bit matrix cores (arith.conv_grad_mode = 'f16x2': fp16 operand "
                         "planes, fp32 accumulation); default: the fp32 backward")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = L.check_arguments(ap, ap.parse_args(argv))
    if a.model != "pipeline":
        raise SystemExit("garmentnets_amd.train_pipeline trains the pipeline model; the first stage's step is python -m garmentnets_amd.train")
    return a


def load_model(a, device):
    """the model to train.  --checkpoint_path: that pipeline checkpoint; neither checkpoint: validate.load_model's seeded synthetic weights; only
    --pointnet2_checkpoint: the second-stage modules keep their constructors' initialisation (under torch.manual_seed(--seed)).  A
    --pointnet2_checkpoint replaces the first stage, and hparams["pointnet2_params"], in every case."""
    from . import synthetic
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
    a = parse_args(argv)
    ranks = L.start(a)
    model = load_model(a, ranks.device).requires_grad_(True).train()
    model.arith = model.arith.replace(device_packs=not a.host_packs)        # (the step reads the model's arithmetic)
    if a.split_backward:
        model.arith = model.arith.replace(conv_grad_mode="f16x2")
    return L.run(STAGE, model, a, ranks)


if __name__ == "__main__":
    L.command(main)
