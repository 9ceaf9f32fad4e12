#!/usr/bin/env python3
"""What hanging a garment costs (DESIGN.md "Hanging garments"; profiles/cloth_time.json).

The garment-sized mesh of tools/winding_time.py (a jittered 51 x 101 sheet: 5151 vertices, 10 000 faces) as a canonical mesh, held at vertex 0, at the
defaults of garmentnets_amd/cloth.py, alone and as a batch of 64, through ops.cloth_simulate_batch: the median of 5 calls after 2 warm-up calls, each
between two events on the stream (the upload of the tables and the read-back of the bad-index flag are inside the interval).  Beside it the numpy
restatement (cloth.simulate_reference) of the same run, timed once on the host, and whether the device gave its bits.  The measurement runs in a child
process under a time limit of its own (--timeout seconds).  Prints one JSON object and writes it to --out.  Not a test and not read by bench.py.
Needs a GPU.

--self_collision (profiles/cloth_collision_time.json) measures the same mesh with the vertex-vertex contacts of cloth.py on, at the defaults of
`simulate --self_collision`: the whole run alone, on the global path and as a batch of 64 (median of --runs calls as above), the list build alone
(gn_cloth_contact_lists on the final state, --list_builds builds between two events, tables already on the device), the mean and the longest list, the
four contact diagnostics, and whether the device gave the restatement's bits over --numpy_substeps substeps (default 8 here: the brute-force lists of
the restatement take seconds a build at this size).

--face_contacts (profiles/cloth_face_contacts_time.json) measures the same mesh with the vertex-face contacts on as well, at the defaults of
`simulate --self_collision --face_contacts`: the whole run alone, on the global path and as a batch of --face_batch garments, the face-list build alone
(gn_cloth_face_contact_lists on the final state, all 5 151 x 10 000 pairs), the lists' lengths, the seven diagnostics, and the restatement's bits over
--numpy_substeps substeps (default 4)."""
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


def measure_contacts(a):
    import torch

    from garmentnets_amd import _lib, cloth, ops
    from garmentnets_amd import simulate as SIM
    verts, faces = sheet()
    params = cloth.ClothParams()
    substeps = cloth.substeps_of(a.duration, params.h)
    g = cloth.garment_from_nocs(verts, faces, 0, REST_SCALE, params)
    on = SIM.collision_params(params, g, {"thickness": None, "margin": None, "rebuild": cloth.DEFAULT_COLLISION_REBUILD,
                                          "max_list": cloth.DEFAULT_COLLISION_MAX_LIST, "relax": cloth.DEFAULT_COLLISION_RELAX})
    g = dataclasses.replace(g, collision=cloth.collision_constants(on))
    out = {"device": torch.cuda.get_device_name(0), "verts": len(verts), "faces": len(faces), "constraints": len(g.l0), "colours": len(g.colour_off) - 1,
           "parameters": dataclasses.asdict(on), "mean_stretch_rest_length": cloth.mean_stretch_rest_length(g), "duration": a.duration,
           "substeps": substeps, "rebuilds": -(-substeps // on.collision_rebuild), "rest_scale": REST_SCALE, "warmup": a.warmup, "runs": a.runs,
           "storage_path": ops.cloth_storage_path(g), "buckets": int(_lib.load().gn_cloth_contact_buckets(len(verts)))}
    state = stats = None
    for label, batch, kw in (("one_garment", 1, {}), ("one_garment_global_path", 1, {"lds_budget": 0}), ("batch_of_64", 64, {})):
        t, (res, st) = device_seconds([g] * batch, substeps, a.warmup, a.runs, stats=True, **kw)
        med = statistics.median(t)
        out[label] = {"seconds": t, "seconds_median": med, "seconds_per_garment": med / batch, "microseconds_per_substep": med / substeps * 1e6}
        if state is None:
            state, stats = tuple(r.cpu().numpy() for r in res[0]), st[0]
        else:
            out[label]["same_bits_as_one_garment"] = all(bool(np.array_equal(r.cpu().numpy(), s)) for got in res for r, s in zip(got, state))
            out[label]["same_diagnostics_as_one_garment"] = all(d == stats for d in st)
    out["contact_diagnostics"] = stats
    out["diagnostics"] = cloth.diagnostics(g, *state)
    # the list build alone, on the final state
    dev = torch.device("cuda", torch.cuda.current_device())
    col = ops.cloth_collision_constants([g], "cloth_time")
    for label, batch in (("list_build", 1), ("list_build_batch_of_64", 64)):
        tab = ops.cloth_device_tables([g] * batch, [state] * batch, dev)
        buf = ops.cloth_contact_buffers([g] * batch, tab, col, dev)
        times = []
        for i in range(a.warmup + a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.list_builds):
                ops._cloth_lists_call(tab, buf, col, batch, _lib.CLOTH_LISTS_BUILD | _lib.CLOTH_LISTS_TRAVEL)
            t1.record()
            t1.synchronize()
            if i >= a.warmup:
                times.append(t0.elapsed_time(t1) * 1e-3 / a.list_builds)
        out[label] = {"builds_per_interval": a.list_builds, "seconds": times, "microseconds_median": statistics.median(times) * 1e6}
        if batch == 1:
            n, total = buf["list_n"].cpu().numpy(), buf["list_total"].cpu().numpy()
            out["lists_of_the_final_state"] = {"mean_length": float(n.mean()), "longest": int(total.max()), "cut": int((total - n).sum())}
    counts, overflow = (t.cpu().numpy() for t in ops.cloth_contact_lists([g])[0][1:])
    out["lists_of_the_start_pose"] = {"mean_length": float(counts.mean()), "longest": int((counts + overflow).max())}
    if a.numpy_substeps != 0:
        n = 8 if a.numpy_substeps < 0 else a.numpy_substeps
        t0 = time.perf_counter()
        ref = cloth.simulate_reference(g, n, stats=True)
        dt = time.perf_counter() - t0
        got, st = ops.cloth_simulate_batch([g], n, stats=True)
        out["numpy_restatement"] = {"substeps": n, "seconds": dt, "microseconds_per_substep": dt / n * 1e6, "device_gave_the_same_bits": bool(
            np.array_equal(ref[0], got[0][0].cpu().numpy()) and np.array_equal(ref[1], got[0][1].cpu().numpy()) and ref[2] == st[0])}
    return out


def measure_face_contacts(a):
    import torch

    from garmentnets_amd import cloth, ops
    from garmentnets_amd import simulate as SIM
    verts, faces = sheet()
    params = cloth.ClothParams()
    substeps = cloth.substeps_of(a.duration, params.h)
    g = cloth.garment_from_nocs(verts, faces, 0, REST_SCALE, params)
    on = SIM.collision_params(params, g, {"thickness": None, "margin": None, "rebuild": cloth.DEFAULT_COLLISION_REBUILD,
                                          "max_list": cloth.DEFAULT_COLLISION_MAX_LIST, "relax": cloth.DEFAULT_COLLISION_RELAX,
                                          "face": {"thickness": None, "max_list": cloth.DEFAULT_FACE_MAX_LIST}})
    g = dataclasses.replace(g, collision=cloth.collision_constants(on), face_collision=cloth.face_collision_constants(on))
    out = {"device": torch.cuda.get_device_name(0), "verts": len(verts), "faces": len(faces), "pairs_per_build": len(verts) * len(faces),
           "constraints": len(g.l0), "parameters": dataclasses.asdict(on), "mean_stretch_rest_length": cloth.mean_stretch_rest_length(g),
           "duration": a.duration, "substeps": substeps, "rebuilds": -(-substeps // on.collision_rebuild), "rest_scale": REST_SCALE, "warmup": a.warmup,
           "runs": a.runs, "storage_path": ops.cloth_storage_path(g),
           "face_chunks": ops.cloth_face_chunks(1, len(verts), len(faces), len(verts), on.face_max_list)}
    state = stats = None
    for label, batch, kw in (("one_garment", 1, {}), ("one_garment_global_path", 1, {"lds_budget": 0}), (f"batch_of_{a.face_batch}", a.face_batch, {})):
        t, (res, st) = device_seconds([g] * batch, substeps, a.warmup, a.runs, stats=True, **kw)
        med = statistics.median(t)
        out[label] = {"seconds": t, "seconds_median": med, "seconds_per_garment": med / batch, "microseconds_per_substep": med / substeps * 1e6}
        if state is None:
            state, stats = tuple(r.cpu().numpy() for r in res[0]), st[0]
        else:
            out[label]["same_bits_as_one_garment"] = all(bool(np.array_equal(r.cpu().numpy(), s)) for got in res for r, s in zip(got, state))
            out[label]["same_diagnostics_as_one_garment"] = all(d == stats for d in st)
    out["contact_diagnostics"] = stats
    out["diagnostics"] = cloth.diagnostics(g, *state)
    # the face-list build alone, on the final state
    dev = torch.device("cuda", torch.cuda.current_device())
    col, fcol = ops.cloth_collision_constants([g], "cloth_time"), ops.cloth_face_collision_constants([g], "cloth_time")
    for label, batch in (("face_list_build", 1), (f"face_list_build_batch_of_{a.face_batch}", a.face_batch)):
        tab = ops.cloth_device_tables([g] * batch, [state] * batch, dev)
        buf = ops.cloth_face_buffers([g] * batch, tab, fcol, dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        times = []
        for i in range(a.warmup + a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.list_builds):
                ops._cloth_face_lists_call(tab, buf, col, fcol, batch, bad)
            t1.record()
            t1.synchronize()
            if i >= a.warmup:
                times.append(t0.elapsed_time(t1) * 1e-3 / a.list_builds)
        med = statistics.median(times)
        out[label] = {"builds_per_interval": a.list_builds, "chunks": buf["chunks"], "seconds": times, "microseconds_median": med * 1e6,
                      "pairs_per_second": batch * len(verts) * len(faces) / med}
        if batch == 1:
            n, total = buf["list_n"].cpu().numpy(), buf["list_total"].cpu().numpy()
            out["face_lists_of_the_final_state"] = {"mean_length": float(n.mean()), "longest": int(total.max()), "cut": int((total - n).sum())}
    counts, overflow = (t.cpu().numpy() for t in ops.cloth_face_contact_lists([g])[0][1:])
    out["face_lists_of_the_start_pose"] = {"mean_length": float(counts.mean()), "longest": int((counts + overflow).max())}
    if a.numpy_substeps != 0:
        n = 4 if a.numpy_substeps < 0 else a.numpy_substeps
        t0 = time.perf_counter()
        ref = cloth.simulate_reference(g, n, stats=True)
        dt = time.perf_counter() - t0
        got, st = ops.cloth_simulate_batch([g], n, stats=True)
        out["numpy_restatement"] = {"substeps": n, "seconds": dt, "microseconds_per_substep": dt / n * 1e6, "device_gave_the_same_bits": bool(
            np.array_equal(ref[0], got[0][0].cpu().numpy()) and np.array_equal(ref[1], got[0][1].cpu().numpy()) and ref[2] == st[0])}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="default profiles/cloth_time.json, with --self_collision profiles/cloth_collision_time.json, with "
                                                "--face_contacts profiles/cloth_face_contacts_time.json")
    ap.add_argument("--self_collision", action="store_true", help="measure the run with contacts on instead")
    ap.add_argument("--face_contacts", action="store_true", help="measure the run with vertex and vertex-face contacts on instead")
    ap.add_argument("--face_batch", type=int, default=16, help="garments of the batch row (--face_contacts)")
    ap.add_argument("--list_builds", type=int, default=50, help="list builds between two events (--self_collision, --face_contacts)")
    ap.add_argument("--duration", type=float, default=3.0, help="seconds simulated (the default of garmentnets_amd.simulate)")
    ap.add_argument("--numpy_substeps", type=int, default=-1, help="substeps of the restatement to time (-1: the whole run, 0: none)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=420.0, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.out is None:
        a.out = ("profiles/cloth_face_contacts_time.json" if a.face_contacts else
                 "profiles/cloth_collision_time.json" if a.self_collision else "profiles/cloth_time.json")
    if a.child:
        print(json.dumps(measure_face_contacts(a) if a.face_contacts else measure_contacts(a) if a.self_collision else measure(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--duration", str(a.duration), "--numpy_substeps", str(a.numpy_substeps),
           "--warmup", str(a.warmup), "--runs", str(a.runs), "--list_builds", str(a.list_builds), "--face_batch", str(a.face_batch)] + (["--self_collision"] if a.self_collision else []) + (
               ["--face_contacts"] if a.face_contacts else [])
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
