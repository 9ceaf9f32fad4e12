"""CPU: the training loop both stages share (garmentnets_amd/train_loop.py) -- the csv's columns and a printed row's keys for both stage records, the two
parsers' defaults, and the order of the calls inside one train_step.  No library call."""
import types

import pytest
import torch

from garmentnets_amd import train as T
from garmentnets_amd import train_loop as L
from garmentnets_amd import train_pipeline as TP

FIRST_METRICS = ["train_loss", "train_nocs_loss", "train_grip_point_loss", "train_nocs_err_dist", "train_grip_point_err_dist"]
SECOND_METRICS = ["train_loss", "train_volume_loss", "train_surface_loss"]


def _model(mc=0.0, device_packs=True):
    """what the stage records read of a model"""
    return types.SimpleNamespace(mc_surface_loss_weight=mc, arith=types.SimpleNamespace(device_packs=device_packs))


# the stage, its model, the timing columns, the metric columns
STAGES = {"first": (T.STAGE, _model(), ["seconds"], FIRST_METRICS),
          "second": (TP.STAGE, _model(), ["data_seconds", "seconds"], SECOND_METRICS),
          "second_mc": (TP.STAGE, _model(mc=1.0), ["data_seconds", "seconds"], SECOND_METRICS + ["train_mc_surface_loss"])}


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("name", list(STAGES))
def test_csv_columns(name, world, resident):
    stage, model, timing, metrics = STAGES[name]
    want = ["epoch", "batch_idx", "garments"] + timing + (["world"] if world > 1 else []) + (["resident"] if resident else []) + metrics
    assert L.csv_columns(stage, model, world, resident) == want
    assert "device_packs" not in want


def test_csv_columns_written_out():
    assert L.csv_columns(T.STAGE, _model(), 1, False) == ["epoch", "batch_idx", "garments", "seconds"] + FIRST_METRICS
    assert L.csv_columns(T.STAGE, _model(), 2, True) == ["epoch", "batch_idx", "garments", "seconds", "world", "resident"] + FIRST_METRICS
    assert L.csv_columns(TP.STAGE, _model(), 1, False) == ["epoch", "batch_idx", "garments", "data_seconds", "seconds"] + SECOND_METRICS
    assert L.csv_columns(TP.STAGE, _model(mc=1.0), 2, True) == (["epoch", "batch_idx", "garments", "data_seconds", "seconds", "world", "resident"]
                                                                + SECOND_METRICS + ["train_mc_surface_loss"])


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("name", list(STAGES))
def test_row_keys(name, world, resident):
    stage, model, timing, metrics = STAGES[name]
    values = {k[len("train_"):]: 0.5 for k in metrics}
    row = L.train_row(stage, model, 3, 1, 2, {"data_seconds": 0.25, "seconds": 0.75}, world, resident, values)
    extras = [] if name == "first" else ["device_packs"]
    want = ["epoch", "batch_idx", "garments"] + timing + extras + (["world"] if world > 1 else []) + (["resident"] if resident else []) + metrics
    assert list(row) == want
    assert (row["epoch"], row["batch_idx"], row["garments"], row["seconds"]) == (3, 1, 2, 0.75)
    assert row.get("data_seconds", 0.25) == 0.25 and row.get("world", 2) == 2 and row.get("resident", True) is True
    assert all(row[k] == 0.5 for k in metrics)
    if extras:
        assert row["device_packs"] is True
    # the csv's columns are the row's keys without the stage's extras
    assert L.csv_columns(stage, model, world, resident) == [k for k in row if k not in extras]


def test_row_reports_the_models_device_packs():
    row = L.train_row(TP.STAGE, _model(device_packs=False), 0, 0, 1, {"data_seconds": 0.0, "seconds": 0.0}, 1, False, {"loss": 1.0})
    assert row["device_packs"] is False


# vars(build_parser().parse_args(["--zarr_in", "x.zarr"])) of the two stages before they shared a loop
COMMON_DEFAULTS = {"model": "pipeline", "checkpoint_path": None, "zarr_in": "x.zarr", "output_dir": ".", "gpu_id": 0, "subset": "train",
                   "static_epoch_seed": False, "dataset_split": (8, 1, 1), "split_seed": 0, "num_batches": None, "num_pc_sample": 6000,
                   "num_volume_sample": 6000, "num_surface_sample": 6000, "num_mc_surface_sample": 0, "surface_sample_ratio": 0.0,
                   "surface_sample_std": 0.05, "volume_size": 128, "volume_group": "nocs_winding_number_field", "tsdf_clip_value": None,
                   "volume_absolute_value": False, "num_views": 4, "random_rot_range": (-180.0, 180.0), "no_augmentation": False,
                   "self_loop_scope": "batch", "grid": 32, "reduce_method": "max", "mc_surface": False, "epochs": 1, "learning_rate": None, "seed": 0,
                   "resident": False, "resident_gib": None, "shuffle": False, "vis_per_items": None, "max_vis_per_epoch_train": None,
                   "max_vis_per_epoch_val": None}
FIRST_DEFAULTS = {**COMMON_DEFAULTS, "batch_size": 8}
SECOND_DEFAULTS = {**COMMON_DEFAULTS, "batch_size": 24, "pointnet2_checkpoint": None, "host_packs": False, "split_backward": False}


@pytest.mark.parametrize("module, want", [(T, FIRST_DEFAULTS), (TP, SECOND_DEFAULTS)])
def test_parser_defaults(module, want):
    assert vars(module.build_parser().parse_args(["--zarr_in", "x.zarr"])) == want


def test_train_step_order():
    calls = []
    model = torch.nn.Linear(3, 2)
    batch = torch.arange(12.0).view(4, 3)
    results = []

    def forward(m, b):
        calls.append("forward")
        assert m is model and b is batch
        results.append({"y": m(b)})
        return results[-1]

    def loss_and_sums(m, b, result):
        calls.append("loss")
        assert result is results[-1] and all(p.grad is None for p in m.parameters())   # (zero_grad(set_to_none=True) came first)
        loss = result["y"].square().sum()
        loss.register_hook(lambda g: calls.append("backward"))
        return loss, loss.detach().double().view(1)

    def metrics_from_sums(m, sums, result, b):
        calls.append("metrics")
        assert result is results[-1] and b is batch
        return {"loss": float(sums[0])}

    class Optimizer:
        def zero_grad(self, set_to_none=False):
            calls.append(("zero_grad", set_to_none))
            for p in model.parameters():
                p.grad = None

        def step(self):
            calls.append("step")
            assert all(p.grad is not None for p in model.parameters())

    class Reducer:
        def reduce(self):
            calls.append("reduce")
            assert all(p.grad is not None for p in model.parameters())

    seen = []
    stage = L.Stage(forward=forward, loss_and_sums=loss_and_sums, metrics_from_sums=metrics_from_sums, metric_keys=lambda m: ("loss",), task_space=False,
                    timing=("seconds",), extras=lambda m: {})
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    with torch.no_grad():
        want = float(model(batch).square().sum())
    metrics = L.train_step(stage, model, Optimizer(), batch, monitor=lambda result: (calls.append("monitor"), seen.append(result)), reducer=Reducer())
    assert calls == [("zero_grad", True), "forward", "loss", "backward", "reduce", "step", "monitor", "metrics"]
    assert len(results) == 1 and len(seen) == 1 and seen[0] is results[0]          # (one forward; the monitor got its very result)
    assert metrics == {"loss": pytest.approx(want, rel=1e-6)}
    # without a monitor and a reducer: the same order with neither of them
    del calls[:]
    L.train_step(stage, model, Optimizer(), batch)
    assert calls == [("zero_grad", True), "forward", "loss", "backward", "step", "metrics"] and len(results) == 2
