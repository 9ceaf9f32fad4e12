#!/usr/bin/env python3
"""What hanging a garment costs (DESIGN.md "Hanging garments"; profiles/cloth_time.json).

The garment-sized mesh of tools/winding_time.py (a jittered 51 x 101 sheet: 5151 vertices, 10 000 faces) as a canonical mesh, held at vertex 0, at the
defaults of garmentnets_amd/cloth.py, alone and as a batch of 64, through ops.cloth_simulate_batch: the median of 5 calls after 2 warm-up calls, each
between two events on the stream (the upload of the tables and the read-back of the bad-index flag are inside the interval).  Beside it the numpy
restatement (cloth.simulate_reference) of the same run, timed once on the host, and whether the device gave its bits.  The measurement runs in a child
process under a time limit of its own (--timeout seconds).  Prints one JSON object and writes it to --out.  Not a test and not read by bench.py.
Needs a GPU."""
import argparse
import dataclasses
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.winding_time import sheet  # noqa: E402

REST_SCALE = 0.9


def device_seconds(garments, substeps, warmup, runs, **kw):
    import torch

    from garmentnets_amd import ops
    times, out = [], None
    for i in range(warmup + runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = ops.cloth_simulate_batch(garments, substeps, **kw)
        t1.record()
        t1.synchronize()
        if i >= warmup:
            times.append(t0.elapsed_time(t1) * 1e-3)
    return times, out


def measure(a):
    import torch

    from garmentnets_amd import cloth, ops
    verts, faces = sheet()
    params = cloth.ClothParams()
    substeps = cloth.substeps_of(a.duration, params.h)
    g = cloth.garment_from_nocs(verts, faces, 0, REST_SCALE, params)
    out = {"device": torch.cuda.get_device_name(0), "verts": len(verts), "faces": len(faces), "constraints": len(g.l0), "stretch": g.n_stretch,
           "bend": g.n_bend, "colours": len(g.colour_off) - 1, "parameters": dataclasses.asdict(params), "duration": a.duration, "substeps": substeps,
           "rest_scale": REST_SCALE, "warmup": a.warmup, "runs": a.runs, "storage_path": ops.cloth_storage_path(g),
           "substeps_per_launch": ops.CLOTH_SUBSTEPS_PER_LAUNCH}
    state = None
    for label, batch, kw in (("one_garment", 1, {}), ("one_garment_global_path", 1, {"lds_budget": 0}), ("one_garment_block_256", 1, {"block": 256}),
                             ("one_garment_block_512", 1, {"block": 512}), ("batch_of_64", 64, {})):
        t, res = device_seconds([g] * batch, substeps, a.warmup, a.runs, **kw)
        med = statistics.median(t)
        out[label] = {"seconds": t, "seconds_median": med, "seconds_per_garment": med / batch, "microseconds_per_substep": med / substeps * 1e6}
        if state is None:
            state = tuple(r.cpu().numpy() for r in res[0])
        else:
            out[label]["same_bits_as_one_garment"] = all(bool(np.array_equal(r.cpu().numpy(), s)) for got in res for r, s in zip(got, state))
    out["diagnostics"] = cloth.diagnostics(g, *state)
    if a.numpy_substeps != 0:
        n = substeps if a.numpy_substeps < 0 else a.numpy_substeps
        t0 = time.perf_counter()
        ref = cloth.simulate_reference(g, n)
        dt = time.perf_counter() - t0
        out["numpy_restatement"] = {"substeps": n, "seconds": dt, "microseconds_per_substep": dt / n * 1e6}
        if n == substeps:
            out["numpy_restatement"]["device_gave_the_same_bits"] = bool(np.array_equal(ref[0], state[0]) and np.array_equal(ref[1], state[1]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="profiles/cloth_time.json")
    ap.add_argument("--duration", type=float, default=3.0, help="seconds simulated (the default of garmentnets_amd.simulate)")
    ap.add_argument("--numpy_substeps", type=int, default=-1, help="substeps of the restatement to time (-1: the whole run, 0: none)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=420.0, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--duration", str(a.duration), "--numpy_substeps", str(a.numpy_substeps),
           "--warmup", str(a.warmup), "--runs", str(a.runs)]
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
