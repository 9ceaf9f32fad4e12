"""python -m garmentnets_amd.validate: score a model on one subset of a dataset store -- the validation_step of the reference's two training
scripts (train_pipeline.py, train_pointnet2.py; the metrics of ConvImplicitWNFPipeline.infer / PointNet2NOCS.infer), without Lightning.

Writes to --output_dir:
  val_metrics.csv   one row per batch: batch_idx, garments, seconds, every val_* metric of that batch
  summary.json      the epoch values, the number of batches / garments and the wall time

Epoch value (the definition used here): the mean of the per-batch values weighted by the garments of each batch.  Lightning 1.4 weights its
epoch mean of a logged value by a batch size it infers from the batch; what it infers from a PyG Batch is not pinned, so its number can
differ from this one when the last batch is partial.
"""
import argparse
import csv
import json
import os
import time

import numpy as np
import torch

from . import synthetic
from .io.dataset import GarmentInputDataset

# config/train_pipeline_default.yaml's datamodule keys (batch_size .. split_seed) as command-line defaults
DATAMODULE_DEFAULTS = dict(batch_size=24, num_pc_sample=6000, num_volume_sample=6000, num_surface_sample=6000, num_mc_surface_sample=0,
                           surface_sample_ratio=0.0, surface_sample_std=0.05, volume_size=128, volume_group="nocs_winding_number_field",
                           tsdf_clip_value=None, volume_absolute_value=False, num_views=4, random_rot_range=(-180.0, 180.0),
                           dataset_split=(8, 1, 1), split_seed=0)
EPOCH_DEFINITION = "mean of the per-batch values weighted by the garments of each batch"


def build_parser():
    d = DATAMODULE_DEFAULTS
    ap = argparse.ArgumentParser(description="GarmentNets validation (MI355X-native): the val_* metrics of the reference's validation_step "
                                             "over one subset of a dataset store")
    ap.add_argument("--model", default="pipeline", choices=("pipeline", "pointnet2"),
                    help="pipeline: ConvImplicitWNFPipeline (train_pipeline.py); pointnet2: PointNet2NOCS (train_pointnet2.py)")
    ap.add_argument("--checkpoint_path", default=None, help="Lightning-style .ckpt of that model; default: seeded synthetic weights")
    ap.add_argument("--zarr_in", required=True, help="garmentnets dataset store (Zarr v2)")
    ap.add_argument("--output_dir", default=".")
    ap.add_argument("--gpu_id", type=int, default=0)
    ap.add_argument("--subset", default="val", choices=("val", "test", "train"),
                    help="the data module's seeded instance split; val and test read the store with static_epoch_seed=True, as the "
                         "reference's val_dataset does")
    ap.add_argument("--static_epoch_seed", action="store_true", help="force static_epoch_seed=True for --subset train too")
    ap.add_argument("--dataset_split", type=float, nargs=3, default=d["dataset_split"])
    ap.add_argument("--split_seed", type=int, default=d["split_seed"])
    ap.add_argument("--num_batches", type=int, default=None, help="stop after this many batches")
    ap.add_argument("--batch_size", type=int, default=d["batch_size"])
    ap.add_argument("--num_pc_sample", type=int, default=d["num_pc_sample"])
    ap.add_argument("--num_volume_sample", type=int, default=d["num_volume_sample"])
    ap.add_argument("--num_surface_sample", type=int, default=d["num_surface_sample"])
    ap.add_argument("--num_mc_surface_sample", type=int, default=d["num_mc_surface_sample"])
    ap.add_argument("--surface_sample_ratio", type=float, default=d["surface_sample_ratio"])
    ap.add_argument("--surface_sample_std", type=float, default=d["surface_sample_std"])
    ap.add_argument("--volume_size", type=int, default=d["volume_size"])
    ap.add_argument("--volume_group", default=d["volume_group"])
    ap.add_argument("--tsdf_clip_value", type=float, default=d["tsdf_clip_value"])
    ap.add_argument("--volume_absolute_value", action="store_true")
    ap.add_argument("--num_views", type=int, default=d["num_views"])
    ap.add_argument("--random_rot_range", type=float, nargs=2, default=d["random_rot_range"])
    ap.add_argument("--no_augmentation", action="store_true", help="datamodule.enable_augumentation=False (the configs: True)")
    ap.add_argument("--self_loop_scope", default="batch", choices=("batch", "example"),
                    help="PointConv's self loops on a batched graph: batch (default) = PyG's literal behaviour, what the reference's "
                         "validation_step computes; example = every garment as in a batch of one")
    ap.add_argument("--grid", type=int, default=32, help="synthetic weights: the volume grid")
    ap.add_argument("--reduce_method", default="max", help="synthetic weights: the gridding reduction")
    ap.add_argument("--mc_surface", action="store_true", help="synthetic weights: with the mc-surface decoder (mc_surface_loss_weight 1)")
    return ap


def make_dataset(a, volume_task_space=False):
    """the subset's dataset with the datamodule keys of `a`; the pointnet2 model reads no targets (train_pointnet2_default.yaml: 0 samples)"""
    targets = a.model == "pipeline"
    return GarmentInputDataset(a.zarr_in, num_pc_sample=a.num_pc_sample, num_views=a.num_views,
                               static_epoch_seed=a.static_epoch_seed or a.subset in ("val", "test"),
                               enable_augumentation=not a.no_augmentation, random_rot_range=tuple(a.random_rot_range),
                               volume_task_space=volume_task_space, dataset_split=tuple(a.dataset_split), split_seed=a.split_seed,
                               num_volume_sample=a.num_volume_sample if targets else 0,
                               num_surface_sample=a.num_surface_sample if targets else 0,
                               num_mc_surface_sample=a.num_mc_surface_sample if targets else 0,
                               surface_sample_ratio=a.surface_sample_ratio, surface_sample_std=a.surface_sample_std, volume_size=a.volume_size,
                               volume_group=a.volume_group, tsdf_clip_value=a.tsdf_clip_value, volume_absolute_value=a.volume_absolute_value)


def host_batches(dataset, indices, batch_size):
    """-> (dataset indices, collated host Batch) per batch of the subset, in order (the reference's val_dataloader: shuffle=False)"""
    for i in range(0, len(indices), batch_size):
        chunk = [int(k) for k in indices[i:i + batch_size]]
        yield chunk, GarmentInputDataset.collate([dataset[k] for k in chunk])


def epoch_values(rows):
    """{key: garment-weighted mean} over the per-batch rows (dicts with "garments" and the val_* keys)"""
    w = np.array([r["garments"] for r in rows], dtype=np.float64)
    keys = [k for k in rows[0] if k.startswith("val_")] if rows else []
    return {k: float(np.sum(w * np.array([r[k] for r in rows], dtype=np.float64)) / np.sum(w)) for k in keys}


def load_model(a, device):
    from .networks.conv_implicit_wnf import ConvImplicitWNFPipeline
    from .networks.pointnet2_nocs import PointNet2NOCS
    if a.model == "pipeline":
        if a.checkpoint_path:
            model = ConvImplicitWNFPipeline.load_from_checkpoint(a.checkpoint_path)
        else:
            hp = synthetic.default_hparams(grid=a.grid, reduce_method=a.reduce_method, mc_surface=a.mc_surface)
            model = ConvImplicitWNFPipeline(**hp)
            model.load_state_dict(synthetic.synthetic_state_dict(hp, 0))
        model.pointnet2_nocs.set_self_loop_scope(a.self_loop_scope)
    else:
        if a.checkpoint_path:
            model = PointNet2NOCS.load_from_checkpoint(a.checkpoint_path)
        else:
            hp = synthetic.default_hparams()
            model = PointNet2NOCS(**hp["pointnet2_params"])
            prefix = "pointnet2_nocs."
            model.load_state_dict({k[len(prefix):]: v for k, v in synthetic.synthetic_state_dict(hp, 0).items() if k.startswith(prefix)})
        model.set_self_loop_scope(a.self_loop_scope)
    return model.to(device).eval().requires_grad_(False)


def write_outputs(output_dir, rows, summary):
    os.makedirs(output_dir, exist_ok=True)
    cols = ["batch_idx", "garments", "seconds"] + sorted({k for r in rows for k in r if k.startswith("val_")})
    with open(os.path.join(output_dir, "val_metrics.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=cols)
        w.writeheader()
        for r in rows:
            w.writerow({k: r.get(k, "") for k in cols})
    with open(os.path.join(output_dir, "summary.json"), "w") as f:
        json.dump(summary, f, indent=2)


def validation_rows(model, dataset, indices, batch_size, num_batches, device, log=None, batches=None, hook=None):
    """the validation loop: one row (batch_idx, garments, seconds, every val_* metric) per batch of `indices`, at most num_batches of them.
    batches: another source of (dataset indices, Batch) pairs than host_batches(dataset, indices, batch_size), e.g. ResidentDataset.batches(...).
    hook: called as hook(batch_idx, batch on the device, the model's forward of it) after each batch's metrics, which are then formed from that one
    forward (train_loop.py's validation monitors)"""
    rows = []
    for batch_idx, (chunk, batch) in enumerate(host_batches(dataset, indices, batch_size) if batches is None else batches):
        if num_batches is not None and batch_idx >= num_batches:
            break
        t0 = time.time()
        with torch.no_grad():
            if hook is None:
                metrics = model.validation_metrics(batch.to(device))
            else:
                on_device = batch.to(device)
                result = model(on_device)
                metrics = model.validation_metrics(on_device, result=result)
                hook(batch_idx, on_device, result)
        row = {"batch_idx": batch_idx, "garments": len(chunk), "seconds": time.time() - t0}
        row.update({"val_" + k: float(v) for k, v in metrics.items()})
        rows.append(row)
        if log is not None:
            log(row)
    return rows


def main(argv=None):
    a = build_parser().parse_args(argv)
    device = torch.device("cuda:{}".format(a.gpu_id))
    torch.cuda.set_device(device)
    model = load_model(a, device)
    dataset = make_dataset(a, volume_task_space=getattr(model, "volume_task_space", False))
    indices = dataset.subset_indices(a.subset)
    t_start = time.time()
    rows = validation_rows(model, dataset, indices, a.batch_size, a.num_batches, device, log=lambda row: print(json.dumps(row)))
    wall = time.time() - t_start
    summary = {"model": a.model, "subset": a.subset, "batches": len(rows), "garments": int(sum(r["garments"] for r in rows)),
               "epoch": epoch_values(rows), "epoch_definition": EPOCH_DEFINITION, "wall_seconds": wall,
               "seconds_per_batch": (float(np.mean([r["seconds"] for r in rows])) if rows else None)}
    write_outputs(a.output_dir, rows, summary)
    print(json.dumps(summary["epoch"]))
    return summary


if __name__ == "__main__":
    main()
