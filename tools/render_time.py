#!/usr/bin/env python3
"""What the monitor images of one training batch cost (DESIGN.md "Training monitors"; profiles/render_time.json).

The image pairs of the second stage's vis_batch with every garment of a batch selected: 24 garments, each a NOCS pair of 6000 points with its two grip
points and a WNF slice pair of 6000 queries, S = 256, kernel 4 -- 96 images -- two ways on the same host, from the same image specs:

  device   visualize.render_batch(backend="device"): the inputs already on the device, one launch pair, the finished images copied to the host
           (the interval ends when they are there)
  numpy    visualize.render_batch(backend="numpy"): the host restatement, the inputs already on the host

alternating device, numpy, ...: 2 warm-up runs of each, then the median of 5 runs of each.  The two results are compared for equality.  The
measurement runs in a child process under a time limit of its own (--timeout seconds).  Prints one JSON object and writes it to --out.  Not a test
and not read by bench.py.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def batch_specs(V, garments, points, queries, to):
    """the specs of one batch, every tensor through `to` (upload or identity)"""
    import numpy as np
    rng = np.random.RandomState(0)
    specs = []
    for _ in range(garments):
        gt = rng.rand(points, 3).astype(np.float32)
        pred = np.clip(gt + rng.randn(points, 3).astype(np.float32) * np.float32(0.03), 0, 1).astype(np.float32)
        q = rng.rand(queries, 3).astype(np.float32)
        w = (rng.rand(queries) * 2 - 0.5).astype(np.float32)
        specs += V.nocs_pair_specs(to(gt), to(pred), to(gt[0]), to(pred[0]))
        specs += V.wnf_pair_specs(to(q), to(w), to((w + np.float32(0.1)).astype(np.float32)))
    return specs


def measure(a):
    import numpy as np
    import torch

    from garmentnets_amd import visualize as V
    dev = torch.device("cuda", 0)
    on_device = batch_specs(V, a.garments, a.points, a.queries, lambda x: torch.from_numpy(x).to(dev))
    on_host = batch_specs(V, a.garments, a.points, a.queries, lambda x: x)
    times = {"device": [], "numpy": []}
    last = {}
    for i in range(a.warmup + a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last["device"] = V.render_batch(on_device, a.size, "device")
        t1 = time.perf_counter()
        last["numpy"] = V.render_batch(on_host, a.size, "numpy")
        t2 = time.perf_counter()
        if i >= a.warmup:
            times["device"].append(t1 - t0)
            times["numpy"].append(t2 - t1)
    out = {"device_name": torch.cuda.get_device_name(0), "garments": a.garments, "points": a.points, "queries": a.queries, "img_size": a.size,
           "images": len(on_device), "warmup": a.warmup, "runs": a.runs, "order": "device, numpy, device, numpy, ...",
           "equal": bool(np.array_equal(last["device"], last["numpy"]))}
    for k, t in times.items():
        out[k] = {"seconds": t, "seconds_median": statistics.median(t), "seconds_min": min(t), "seconds_max": max(t)}
    out["numpy_over_device"] = out["numpy"]["seconds_median"] / out["device"]["seconds_median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="profiles/render_time.json")
    ap.add_argument("--garments", type=int, default=24)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--queries", type=int, default=6000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for k in ("garments", "points", "queries", "size", "warmup", "runs")
                                                                     for x in ("--" + k, str(getattr(a, k)))]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
    if res.returncode != 0:
        return res.returncode
    out = json.loads(res.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
