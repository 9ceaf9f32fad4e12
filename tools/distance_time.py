#!/usr/bin/env python3
"""What the distance field of a garment costs (DESIGN.md "Distance, signed-distance and occupancy targets"; profiles/distance_time.json).

The garment-sized mesh of tools/winding_time.py (a jittered 51 x 101 sheet: 5151 vertices, 10 000 faces) at 128^3, two ways in one process:

  lattice   ops.distance_field_batch: the kernel forms the lattice, a thread owns 4 nodes
  points    ops.point_mesh_sqdist on the lattice points, uploaded beforehand: one node per thread (the only way to these numbers before the
            lattice kernel existed)

alternating lattice, points, lattice, points ...: 2 warm-up launches of each, then the median of 5 launches of each, every launch between two
events on the stream.  The two results are compared for equality.  The measurement runs in a child process under a time limit of its own
(--timeout seconds).  Prints one JSON object and writes it to --out.  Not a test and not read by bench.py.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.winding_time import sheet  # noqa: E402


def measure(a):
    import torch

    from garmentnets_amd import ops, winding
    verts, faces = sheet()
    dev = torch.device("cuda", 0)
    mesh = (torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev))
    shape = (a.size,) * 3
    points = torch.from_numpy(winding.lattice_points(shape)).to(dev)
    ways = {"lattice": lambda: ops.distance_field_batch([mesh], shape), "points": lambda: ops.point_mesh_sqdist(points, *mesh)}
    times = {k: [] for k in ways}
    last = {}
    for i in range(a.warmup + a.runs):
        for k, launch in ways.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            last[k] = launch()                              # (the bad-index flag is read back after the launch: inside the interval)
            t1.record()
            t1.synchronize()
            if i >= a.warmup:
                times[k].append(t0.elapsed_time(t1) * 1e-3)
    d2, face_idx = last["lattice"]
    p_idx, p_d2 = last["points"]
    pairs = a.size ** 3 * len(faces)
    out = {"device": torch.cuda.get_device_name(0), "verts": len(verts), "faces": len(faces), "volume_size": a.size, "warmup": a.warmup,
           "runs": a.runs, "pairs": pairs, "order": "lattice, points, lattice, points, ...",
           "equal": bool(torch.equal(d2.reshape(-1), p_d2) and torch.equal(face_idx.reshape(-1), p_idx))}
    for k, t in times.items():
        med = statistics.median(t)
        out[k] = {"seconds": t, "seconds_median": med, "seconds_min": min(t), "seconds_max": max(t), "pairs_per_second": pairs / med}
    out["points_over_lattice"] = out["points"]["seconds_median"] / out["lattice"]["seconds_median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="profiles/distance_time.json")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--warmup", str(a.warmup), "--runs", str(a.runs)]
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
