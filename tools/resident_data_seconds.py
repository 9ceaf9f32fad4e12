#!/usr/bin/env python3
"""What a batch costs the host, from the host dataset and from the resident one (DESIGN.md "Resident dataset"; profiles/resident_data_seconds.json).

  --write_store PATH          a synthetic dataset store of the shipped sizes: 48 samples of 4 x 8000-point views, a 5000-vertex / 10000-face mesh and a
                              128^3 fp32 volume in zlib-1 chunks.  Synthetic arrays compress unlike the real Blosc store: the host path's inflate time is
                              this store's, not the real one's.
  --summarise_csv CSV         the medians of a train_metrics.csv of `python -m garmentnets_amd.train_pipeline` (of any commit: the parent's host run)
  --resident_run STORE        train_pipeline with --resident over STORE (two epochs, batch 24, 6000 / 6000 / 6000), its medians, the one-off load time and
                              nbytes, and the summed device time of the gn_resident_* launches of a batch, each launch between two events on the stream
  --exact_targets             with --resident_run: the run takes gt_volume_value from the meshes (--exact_targets; the store's volumes are not read)
Every mode prints one JSON object; --out FILE merges it into FILE under --label.  Not a test and not read by bench.py.  The runs need a GPU."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RUN_ARGS = ["--epochs", "2", "--batch_size", "24", "--num_pc_sample", "6000", "--num_volume_sample", "6000", "--num_surface_sample", "6000"]
LAUNCHES = ("resident_points", "resident_garment", "resident_volume", "resident_volume_queries", "resident_query_targets", "resident_surface",
            "resident_mc_surface")


def write_store(path, samples=48, views=(8000,) * 4, verts=5000, faces=10000, volume=128, seed=0):
    from garmentnets_amd.io import zarr_store
    rng = np.random.default_rng(seed)
    root = zarr_store.open_group(path)
    root.require_group("summary").array("cloth_aabb_union", np.array([[-0.4, -0.4, -0.9], [0.4, 0.4, 0.05]], dtype=np.float32))
    ax = np.linspace(0, 1, volume, dtype=np.float32)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    n = sum(views)
    for i in range(samples):
        sg = root.require_group("samples").require_group(f"{i:05d}_Dress_{i:06d}_0")
        sg.put_attrs({"scale": 1.0, "sample_id": f"{i:05d}_Dress", "garment_name": "Dress", "grip_vertex_idx": i})
        pc, mesh = sg.require_group("point_cloud"), sg.require_group("mesh")
        nocs = rng.random((n, 3)).astype(np.float32)
        pc.array("point", (nocs * [0.7, 0.7, 0.9] + [-0.35, -0.35, -0.88]).astype(np.float32), compressor=("zlib", 1))
        pc.array("nocs", nocs, compressor=("zlib", 1))
        pc.array("rgb", rng.integers(0, 256, (n, 3)).astype(np.uint8), compressor=("zlib", 1))
        pc.array("sizes", np.array(views, dtype=np.int64))
        v = rng.random((verts, 3)).astype(np.float32)
        mesh.array("cloth_nocs_verts", v, compressor=("zlib", 1))
        mesh.array("cloth_verts", (v * [0.7, 0.7, 0.9] + [-0.35, -0.35, -0.88]).astype(np.float32), compressor=("zlib", 1))
        mesh.array("cloth_faces_tri", rng.integers(0, verts, (faces, 3)).astype(np.int32), compressor=("zlib", 1))
        # a smooth winding-number-like field plus noise in the low mantissa bits, so that zlib neither collapses it nor stores it raw
        r = 0.2 + 0.1 * rng.random()
        wnf = (1 / (1 + np.exp(-30 * (r - np.sqrt((X - 0.5) ** 2 + (Y - 0.5) ** 2 + (Z - 0.5) ** 2))))).astype(np.float32)
        wnf += (rng.random(wnf.shape, dtype=np.float32) - 0.5) * 1e-3
        sg.require_group("volume").require_group("nocs_winding_number_field").array(str(volume), wnf, chunks=(volume, volume, 16), compressor=("zlib", 1))
    return {"samples": samples, "points": n, "verts": verts, "faces": faces, "volume": volume}


def medians(rows):
    f = lambda k: [float(r[k]) for r in rows]
    return {"rows": len(rows), "garments": [int(r["garments"]) for r in rows], "data_seconds_median": statistics.median(f("data_seconds")),
            "seconds_median": statistics.median(f("seconds")), "data_seconds": f("data_seconds"), "seconds": f("seconds")}


def resident_run(store, output_dir, exact_targets=False):
    import torch
    from garmentnets_amd import ops, train_pipeline
    res = train_pipeline.main(["--zarr_in", store, "--output_dir", output_dir, "--resident"] + (["--exact_targets"] if exact_targets else []) + RUN_ARGS)
    out = medians(res["train_rows"])
    out["exact_targets"] = bool(exact_targets)
    resident, val = res["resident"], res["val_resident"]
    out.update({"load_seconds": resident.load_seconds, "nbytes": resident.nbytes, "val_load_seconds": val.load_seconds, "val_nbytes": val.nbytes,
                "device": torch.cuda.get_device_name(0)})
    # the launches of a batch, each between two events on the stream; one synchronisation per batch, after it
    pairs, real = [], {name: getattr(ops, name) for name in LAUNCHES}

    def bracket(fn):
        def call(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(*args)
            b.record()
            pairs.append((a, b))
        return call
    for name, fn in real.items():
        setattr(ops, name, bracket(fn))
    try:
        per_batch, host = [], []
        chunk = resident.indices[:24]
        for i in range(12):
            del pairs[:]
            t0 = time.perf_counter()
            resident.batch(chunk)
            host.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            if i >= 2:
                per_batch.append(sum(a.elapsed_time(b) for a, b in pairs))
    finally:
        for name, fn in real.items():
            setattr(ops, name, fn)
    out.update({"launches_per_batch": len(pairs), "launch_device_ms_median": statistics.median(per_batch), "launch_device_ms": per_batch,
                "batch_call_seconds_median": statistics.median(host[2:])})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write_store", default=None)
    ap.add_argument("--summarise_csv", default=None)
    ap.add_argument("--resident_run", default=None)
    ap.add_argument("--exact_targets", action="store_true")
    ap.add_argument("--output_dir", default="resident_run_out")
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.write_store:
        t0 = time.time()
        result = write_store(a.write_store)
        result["write_seconds"] = time.time() - t0
    elif a.summarise_csv:
        result = medians(list(csv.DictReader(open(a.summarise_csv))))
    elif a.resident_run:
        result = resident_run(a.resident_run, a.output_dir, a.exact_targets)
    else:
        raise SystemExit("one of --write_store, --summarise_csv, --resident_run")
    result["clock"] = time.strftime("%Y-%m-%d %H:%M:%S %Z")
    print(json.dumps(result))
    if a.out:
        merged = json.load(open(a.out)) if os.path.exists(a.out) else {}
        merged[a.label or "result"] = result
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(merged, indent=2) + "\n")


if __name__ == "__main__":
    main()
