#!/usr/bin/env python3
"""Time the second stage's training step on one MI355X: tools/pipeline_step_time.py [--out FILE.json] [--kernel-stats FILE.csv]

The reference's configuration (train_pipeline_default.yaml): batch 24, 6000 points per garment, 6000 volume and 6000 surface queries, grid 32 with 'max',
synthetic.default_hparams(), synthetic clouds and seeded random targets, the model in training mode (batch-statistics BatchNorm in the aggregator and the
decoders; the first stage frozen).  Reports the median of 20 steps after 5 warm-up steps and the share of the frozen first stage, the aggregator, the
UNet, the heads with the loss, backward and optimizer.step(), each bracketed by events on the stream (tools/train_step_time.py's bracketing), and beside
each the host's own time to issue it.

--kernel-stats FILE.csv --merge: no timing; the kernel_stats csv of a `rocprofv3 --kernel-trace --stats` run of THIS script (a run of its own: the tracer
slows the host) -> the share of the traced kernel time that is not one of this library's kernels (torch's element-wise / copy / fill / reduction
kernels), added to the existing --out file as "foreign_kernels".  Not a test and not read by bench.py.  Needs a GPU: there is no fallback."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from garmentnets_amd import synthetic, train_pipeline as TP  # noqa: E402
from garmentnets_amd.batch import Batch  # noqa: E402
from garmentnets_amd.networks.conv_implicit_wnf import ConvImplicitWNFPipeline  # noqa: E402
from train_step_time import bracketed, summarise  # noqa: E402

PARTS = ("first_stage", "aggregator", "unet", "heads_and_loss", "backward", "optimizer")
# kernels that are not this library's, by the prefixes / name spaces rocprofv3 prints for them
FOREIGN = ("at::", "at_cuda_detail", "__amd_rocclr", "Cijk_", "rocprim", "hipcub", "thrust", "rocblas", "c10::")


def timed_step(model, optimizer, batch, arith=None, host=None):
    optimizer.zero_grad(set_to_none=True)
    s = {}

    def first_stage():
        s["p2"] = TP.first_stage(model, batch)

    def aggregator():
        s["volume"] = TP.aggregate(model, s["p2"]["nocs_data"])

    def unet():
        s["u3"] = TP.unet(model, s["volume"], arith)

    def heads_and_loss():
        result = {"pointnet2_result": s["p2"], "unet3d_result": s["u3"], **TP.heads(model, s["u3"], batch)}
        s["loss"] = TP.loss_and_sums(model, batch, result)[0]
    return bracketed([first_stage, aggregator, unet, heads_and_loss, lambda: s["loss"].backward(), optimizer.step], host)


def foreign_share(path):
    """-> the kernel-time share of the kernels that are not this library's, their total and the three largest, from a rocprofv3 kernel_stats csv"""
    total, foreign = 0.0, {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], float(row["TotalDurationNs"])
            total += ns
            bare = name[5:] if name.startswith("void ") else name
            if bare.startswith(FOREIGN) or "at::native" in name:
                foreign[name] = foreign.get(name, 0.0) + ns
    top = sorted(foreign.items(), key=lambda kv: -kv[1])[:3]
    return {"kernel_ms_total": total / 1e6, "foreign_ms_total": sum(foreign.values()) / 1e6, "share": sum(foreign.values()) / total if total else None,
            "largest": [{"name": k[:120], "ms": v / 1e6} for k, v in top]}


def commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--queries", type=int, default=6000)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--strict-fp32-forward", action="store_true", help="the UNet's forward in arith.strict_fp32() instead of the model's arithmetic")
    ap.add_argument("--device-packs", action="store_true", help="the UNet's static weight packs built on the device (arith.device_packs) instead of on the host")
    ap.add_argument("--commit", default=None, help="recorded as it is (default: git rev-parse of the tree, when there is one)")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--merge", action="store_true", help="with --kernel-stats and --out: add the share to the existing file, time nothing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge:
        with open(a.out) as f:
            out = json.load(f)
        out["foreign_kernels"] = foreign_share(a.kernel_stats)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=2) + "\n")
        print(json.dumps(out["foreign_kernels"]))
        return
    if not torch.cuda.is_available():
        raise SystemExit("pipeline_step_time.py needs a GPU")
    dev = torch.device("cuda:0")
    hp = synthetic.default_hparams(grid=a.grid, reduce_method="max")
    model = ConvImplicitWNFPipeline(**hp)
    model.load_state_dict(synthetic.synthetic_state_dict(hp, 0, planted_nocs=True))     # (the planted NOCS path spreads the points over the cells)
    model = model.to(dev).requires_grad_(True).train()
    x, pos, b = synthetic.synthetic_cloud(a.batch, a.points, seed=0, colour="position")
    g = torch.Generator().manual_seed(0)
    batch = Batch(sizes=[a.points] * a.batch, x=x, pos=pos, batch=b, volume_query_points=torch.rand(a.batch, a.queries, 3, generator=g),
                  gt_volume_value=torch.rand(a.batch, a.queries, generator=g), surf_query_points=torch.rand(a.batch, a.queries, 3, generator=g),
                  gt_sim_points=0.3 * torch.randn(a.batch, a.queries, 3, generator=g)).to(dev)
    opt = model.configure_optimizers()
    if a.device_packs:
        model.arith = model.arith.replace(device_packs=True)
    arith = model.arith.strict_fp32() if a.strict_fp32_forward else None
    rows, host_rows = [], []
    for i in range(a.warmup + a.steps):
        host = []
        t = timed_step(model, opt, batch, arith, host)
        if i >= a.warmup:
            rows.append(t)
            host_rows.append(host)
    second = [p for n, p in model.named_parameters() if not n.startswith("pointnet2_nocs.")]
    out = {"clock": time.strftime("%Y-%m-%d %H:%M:%S %Z"), "commit": a.commit or commit(), "device": torch.cuda.get_device_name(0), "batch": a.batch,
           "points": a.points, "queries": a.queries, "grid": a.grid, "reduce_method": "max", "unet_forward": "fp32" if a.strict_fp32_forward else model.arith.conv_name, "device_packs": model.arith.device_packs, "steps": a.steps, "warmup": a.warmup,
           "trained_parameters": sum(p.numel() for p in second), "trained_tensors": len(second), "parts": list(PARTS)}
    out.update(summarise(rows, PARTS))
    # the host's own time to issue each part: where it is close to the part's stream time, the part is bound by the host, not by its kernels
    out["host_issue_ms_median"] = {n: statistics.median(r[i] for r in host_rows) for i, n in enumerate(PARTS)}
    if a.kernel_stats:
        out["foreign_kernels"] = foreign_share(a.kernel_stats)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=2) + "\n")


if __name__ == "__main__":
    main()
