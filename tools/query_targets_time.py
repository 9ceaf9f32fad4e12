#!/usr/bin/env python3
"""What the exact targets of a training batch cost (DESIGN.md "Exact volume targets"; profiles/query_targets_time.json).

The garment-sized mesh of tools/winding_time.py (a jittered 51 x 101 sheet: 5151 vertices, 10 000 faces), B = 24 garments x M = 6000 uniform queries
(1.44e9 pairs), each of the five volume groups two ways in one process:

  new       ops.query_targets_batch: the face chunks are a grid dimension, one fold launch
  baseline  the entries that were there before, on the same inputs widened to fp64 beforehand: ops.winding_number_batch for the groups that read w,
            ops.point_mesh_sqdist_batch for those that read d2, both for the signed distance

alternating new, baseline, new, baseline ...: 2 warm-up rounds, then the median of 5 launches of each, every launch between two events on the stream
(the host work of the operator and its read-back of the bad-index flag are inside the interval, on both sides).  `faster` holds when the new entry's
median is below the baseline's by more than the larger of the two min..max spreads.  The measurement runs in a child process under a time limit of its
own (--timeout seconds).  Prints one JSON object and writes it to --out.  Not a test and not read by bench.py.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.winding_time import sheet  # noqa: E402


def measure(a):
    import numpy as np
    import torch

    from garmentnets_amd import ops, targets
    verts, faces = sheet()
    dev = torch.device("cuda", 0)
    v32 = torch.from_numpy(verts.astype(np.float32)).to(dev)
    f = torch.from_numpy(faces).to(dev)
    q32 = torch.from_numpy(np.random.default_rng(0).random((a.garments, a.queries, 3)).astype(np.float32)).to(dev)
    meshes32 = [(v32, f)] * a.garments
    q64 = [q32[b].double() for b in range(a.garments)]
    meshes64 = [(v32.double(), f)] * a.garments
    pairs = a.garments * a.queries * len(faces)
    out = {"device": torch.cuda.get_device_name(0), "verts": len(verts), "faces": len(faces), "garments": a.garments, "queries": a.queries,
           "face_chunk": targets.face_chunk(), "warmup": a.warmup, "runs": a.runs, "pairs": pairs, "order": "new, baseline, new, baseline, ...", "kinds": {}}
    for kind in targets.KINDS:
        def baseline():
            w = ops.winding_number_batch(q64, meshes64) if targets.needs_w(kind) else None
            d = ops.point_mesh_sqdist_batch(q64, meshes64) if targets.needs_d2(kind) else None
            return w, d
        ways = {"new": lambda: ops.query_targets_batch(q32, meshes32, kind, return_fp64=True), "baseline": baseline}
        times, last = {k: [] for k in ways}, {}
        for i in range(a.warmup + a.runs):
            for k, launch in ways.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                last[k] = launch()
                t1.record()
                t1.synchronize()
                if i >= a.warmup:
                    times[k].append(t0.elapsed_time(t1) * 1e-3)
        _, w, d2, face_idx = last["new"]
        bw, bd = last["baseline"]
        row = {}
        if d2 is not None:
            row["d2_equal"] = bool(all(torch.equal(d2[b], bd[b][1]) and torch.equal(face_idx[b], bd[b][0]) for b in range(a.garments)))
        if w is not None:
            row["w_max_abs_diff"] = float(max((w[b] - bw[b]).abs().max() for b in range(a.garments)))
        for k, t in times.items():
            med = statistics.median(t)
            row[k] = {"seconds": t, "seconds_median": med, "seconds_min": min(t), "seconds_max": max(t), "pairs_per_second": pairs / med}
        spread = max(row[k]["seconds_max"] - row[k]["seconds_min"] for k in ways)
        row["baseline_over_new"] = row["baseline"]["seconds_median"] / row["new"]["seconds_median"]
        row["larger_spread_seconds"] = spread
        row["faster"] = bool(row["baseline"]["seconds_median"] - row["new"]["seconds_median"] > spread)
        out["kinds"][kind] = row
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="profiles/query_targets_time.json")
    ap.add_argument("--garments", type=int, default=24)
    ap.add_argument("--queries", type=int, default=6000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--garments", str(a.garments), "--queries", str(a.queries), "--warmup", str(a.warmup),
           "--runs", str(a.runs)]
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
