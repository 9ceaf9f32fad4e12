#!/usr/bin/env python3
"""Time the first stage's training step on one MI355X: tools/train_step_time.py [--out FILE.json]

The reference's configuration: batch 8, 6000 points per garment, nocs_bins = 64, synthetic clouds (synthetic.synthetic_cloud), the model in
training mode (batch-statistics BatchNorm, dropout).  Reports the median of 20 steps after 5 warm-up steps and the share of forward (with the loss),
backward and optimizer.step(), each bracketed by events on the stream; then the same step with torch.optim.Adam(foreach=True) in FusedAdam's place
(its in-place updates bump the tensor versions the packs are keyed by), the two alternating within one run.  Not a test and not read by bench.py.  Needs a GPU: there is no fallback."""
import argparse
import copy
import json
import statistics
import sys
import os
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from garmentnets_amd import synthetic, train  # noqa: E402
from garmentnets_amd.batch import Batch  # noqa: E402
from garmentnets_amd.networks.pointnet2_nocs import PointNet2NOCS  # noqa: E402
from garmentnets_amd.optim import FusedAdam  # noqa: E402


def bracketed(parts, host=None):
    """run the callables `parts` in order, each between two events on the stream; one synchronisation at the end -> their milliseconds (stream time: it
    holds the host's time wherever the stream waits for the host).  host: a list that receives the host's own milliseconds inside each part (the time
    to issue it, nothing waited for).  tools/pipeline_step_time.py brackets its parts with this too"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(parts) + 1)]
    ev[0].record()
    for i, part in enumerate(parts):
        t0 = time.perf_counter()
        part()
        if host is not None:
            host.append((time.perf_counter() - t0) * 1e3)
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(len(parts))]


def summarise(rows, names):
    """rows: one list of milliseconds per step, a column per name -> the medians, the step's median / min / max and each part's share of it"""
    cols = [[r[i] for r in rows] for i in range(len(names))]
    total = [sum(r) for r in rows]
    med = statistics.median(total)
    out = {"step_ms_median": med, "step_ms_min": min(total), "step_ms_max": max(total)}
    out.update({f"{n}_ms_median": statistics.median(c) for n, c in zip(names, cols)})
    out["share"] = {n: statistics.median(c) / med for n, c in zip(names, cols)}
    return out


def timed_step(model, optimizer, batch):
    optimizer.zero_grad(set_to_none=True)
    state = {}

    def forward():
        state["loss"] = train.loss_and_sums(model, batch)[0]

    return bracketed([forward, lambda: state["loss"].backward(), optimizer.step])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_time.py needs a GPU")
    dev = torch.device("cuda:0")
    hp = synthetic.default_hparams()
    base = PointNet2NOCS(**hp["pointnet2_params"])
    base.load_state_dict({k[len("pointnet2_nocs."):]: v for k, v in synthetic.synthetic_state_dict(hp, 0).items() if k.startswith("pointnet2_nocs.")})
    x, pos, b = synthetic.synthetic_cloud(a.batch, a.points, seed=0)
    g = torch.Generator().manual_seed(0)
    batch = Batch(sizes=[a.points] * a.batch, x=x, pos=pos, batch=b, y=torch.rand(x.shape[0], 3, generator=g),
                  nocs_grip_point=torch.rand(a.batch, 3, generator=g)).to(dev)
    runs = {}
    for name in ("fused", "foreach"):
        model = copy.deepcopy(base).to(dev).train()
        opt = FusedAdam(model, lr=1e-4) if name == "fused" else torch.optim.Adam(model.parameters(), lr=1e-4, foreach=True)
        runs[name] = (model, opt, [])
    torch.manual_seed(0)
    for i in range(a.warmup + a.steps):                 # the two alternate, step by step: the same machine state for both
        for name, (model, opt, rows) in runs.items():
            t = timed_step(model, opt, batch)
            if i >= a.warmup:
                rows.append(t)
    out = {"clock": time.strftime("%Y-%m-%d %H:%M:%S %Z"), "device": torch.cuda.get_device_name(0), "batch": a.batch, "points": a.points,
           "nocs_bins": hp["pointnet2_params"]["nocs_bins"], "steps": a.steps, "warmup": a.warmup,
           "parameters": sum(p.numel() for p in base.parameters()), "tensors": len(list(base.parameters()))}
    for name, (_, _, rows) in runs.items():
        out[name] = summarise(rows, ("forward", "backward", "optimizer"))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=2) + "\n")


if __name__ == "__main__":
    main()
