#!/usr/bin/env python3
"""What one mesh image costs (DESIGN.md "Mesh images"; profiles/mesh_render_time.json).

The mesh: garment 0 of the benchmark's planted batch (bench.bench_inputs: 6000 points, G = 128, mean reduction) through predict_batch at Q = 128 --
the predicted NOCS mesh, coloured by its own coordinates, seen from the front.  The interval: ONE launch pair, ops.render_mesh_batch then
ops.color_mesh_batch, between two events on the stream, the inputs resident and the images left on the device.  Per image size: --warmup pairs, then
the median of --runs pairs, each timed on its own.  The device's images are compared with the numpy restatement's once (--no-check skips it).
Prints one JSON object and writes it to --out.  Not a test and not read by bench.py.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="profiles/mesh_render_time.json")
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--volume-size", type=int, default=128)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from garmentnets_amd import ops, visualize as V
    from garmentnets_amd.batch import Batch
    from garmentnets_amd.networks.conv_implicit_wnf import ConvImplicitWNFPipeline
    from garmentnets_amd.predict import predict_batch
    dev = torch.device("cuda", 0)
    hp, sd, shard, _ = bench.bench_inputs(1, a.points, a.grid, "mean", "planted")
    model = ConvImplicitWNFPipeline(**hp)
    model.load_state_dict(sd)
    model = model.to(dev).eval().requires_grad_(False)
    data = Batch(sizes=shard.sizes, x=shard.x, pos=shard.pos, batch=shard.batch).to(dev)
    res = predict_batch(model, data, volume_size=a.volume_size, iso_surface_level=0.5, gradient_sigma=0.5, gradient_direction="ascent")[0]
    verts = res["verts"].to(torch.float32).contiguous()
    faces = res["faces"].to(torch.int32).contiguous()
    colors = torch.cat([verts, verts.new_ones((verts.shape[0], 1))], dim=1).contiguous()
    vseg, fseg = [0, verts.shape[0]], [0, faces.shape[0]]
    out = {"device_name": torch.cuda.get_device_name(0), "mesh": "garment 0 of bench.bench_inputs(1, %d, %d, 'mean', 'planted') at Q = %d, NOCS vertices"
           % (a.points, a.grid, a.volume_size), "verts": int(verts.shape[0]), "faces": int(faces.shape[0]), "side": "front", "warmup": a.warmup,
           "runs": a.runs, "interval": "events around one render_mesh_batch + color_mesh_batch pair", "sizes": {}}

    def pair(S):
        idx = ops.render_mesh_batch(verts, faces, vseg, fseg, ["front"], S)
        return idx, ops.color_mesh_batch(idx, verts, faces, colors, vseg, fseg, ["front"])

    for S in a.sizes:
        for _ in range(a.warmup):
            pair(S)
        ms = []
        for _ in range(a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            idx, img = pair(S)
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        row = {"ms": ms, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
               "covered_pixels": int((idx != -1).sum())}
        if not a.no_check:
            want = V.render_mesh_batch([V.mesh_spec(verts.cpu().numpy(), faces.cpu().numpy(), colors.cpu().numpy())], S, "numpy")[0]
            row["equal_numpy"] = bool(np.array_equal(img[0].cpu().numpy().view(np.uint32), want.view(np.uint32)))
        out["sizes"][str(S)] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
