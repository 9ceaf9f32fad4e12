#!/usr/bin/env python3
"""What the winding-number field of a garment costs (DESIGN.md "Winding numbers"; profiles/winding_time.json).

One garment-sized mesh (a jittered 51 x 101 sheet: 5151 vertices, 10 000 faces) at 128^3, alone and as a batch of four, through
ops.winding_field_batch: the median of 5 launches after 2 warm-up launches, each between two events on the stream.  Beside it, for scale, the numpy
reference (winding.winding_field_reference) on the same mesh at 32^3, timed once on the host.  The measurement runs in a child process under a
time limit of its own (--timeout seconds).  Prints one JSON object and writes it to --out.  Not a test and not read by bench.py.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# per (query, face) pair, csrc/winding.hip wn_omega + the accumulation: 9 subtractions, 7 three-term dot products (5 each), the cross product (9),
# the denominator (5 multiplications, 3 additions), the doubling and the running sum -- all plain fp64 add / mul -- plus 3 sqrt and 1 atan2
PLAIN_OPS_PER_PAIR = 9 + 7 * 5 + 9 + 8 + 1 + 1
# MI355X: 78.6 TFLOP/s of vector fp64 counts an fma as two; a kernel that may not fuse issues at most half of that in plain operations
FP64_VECTOR_PLAIN_OPS_PER_SECOND = 78.6e12 / 2


def sheet(n=51, m=101, seed=0):
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(0.05, 0.95, n), np.linspace(0.05, 0.95, m), indexing="ij")
    z = 0.5 + 0.2 * np.sin(4.7 * u) * np.cos(5.3 * v)
    verts = np.stack([u, v, z], axis=-1).reshape(-1, 3) + rng.uniform(-1e-3, 1e-3, (n * m, 3))
    idx = np.arange(n * m).reshape(n, m)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], axis=1).reshape(-1, 3).astype(np.int32)
    return verts, faces


def device_seconds(meshes, size, warmup, runs):
    import torch

    from garmentnets_amd import ops
    times = []
    for i in range(warmup + runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        ops.winding_field_batch(meshes, (size,) * 3)        # (its bad-index flag is read back after the launch: inside the interval)
        t1.record()
        t1.synchronize()
        if i >= warmup:
            times.append(t0.elapsed_time(t1) * 1e-3)
    return times


def measure(a):
    import torch

    from garmentnets_amd import winding
    verts, faces = sheet()
    dev = torch.device("cuda", 0)
    mesh = (torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev))
    out = {"device": torch.cuda.get_device_name(0), "verts": len(verts), "faces": len(faces), "volume_size": a.size, "warmup": a.warmup,
           "runs": a.runs, "plain_fp64_ops_per_pair": PLAIN_OPS_PER_PAIR, "sqrt_per_pair": 3, "atan2_per_pair": 1}
    for label, batch in (("one_garment", 1), ("batch_of_four", 4)):
        t = device_seconds([mesh] * batch, a.size, a.warmup, a.runs)
        pairs = batch * a.size ** 3 * len(faces)
        med = statistics.median(t)
        out[label] = {"seconds": t, "seconds_median": med, "pairs": pairs, "pairs_per_second": pairs / med,
                      "plain_fp64_ops_per_second": pairs * PLAIN_OPS_PER_PAIR / med,
                      "fraction_of_fp64_vector_rate_without_fma": pairs * PLAIN_OPS_PER_PAIR / med / FP64_VECTOR_PLAIN_OPS_PER_SECOND}
    t0 = time.perf_counter()
    ref = winding.winding_field_reference(verts, faces, (a.numpy_size,) * 3)
    dt = time.perf_counter() - t0
    got = winding.winding_field([(verts, faces)], (a.numpy_size,) * 3)[0]
    out["numpy_reference"] = {"volume_size": a.numpy_size, "seconds": dt, "pairs": a.numpy_size ** 3 * len(faces),
                              "pairs_per_second": a.numpy_size ** 3 * len(faces) / dt,
                              "max_abs_difference_of_the_device_field": float(np.abs(got.astype(np.float64) - ref).max())}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="profiles/winding_time.json")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--numpy_size", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=420.0, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--numpy_size", str(a.numpy_size), "--warmup", str(a.warmup),
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
