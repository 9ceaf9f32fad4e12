#!/usr/bin/env python3
"""What one launch set of the point clouds from meshes costs (DESIGN.md "Point clouds from meshes"; profiles/point_cloud_time.json).

The meshes: --garments wavy open tubes ("dresses") of 100 x 51 vertices and 10 000 faces each, the mesh size of the shipped stores, inside the
synthetic stores' cloth_aabb_union; the cameras: point_cloud.camera_ring's defaults, --views of them at --size pixels.  The interval: ONE launch set,
ops.depth_render_batch then ops.depth_cloud (the row counts and their scan, the per-image sizes read back to size the outputs, the write pass), between
two events on the stream, the meshes resident and the clouds left on the device; --warmup sets, then the median of --runs sets, each timed on its own.
The numpy restatement's wall time on the host is taken once, as context, and its arrays are compared with the device's.  Prints one JSON object and
writes it to --out.  Not a test and not read by bench.py.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AABB = [[-0.4, -0.4, -0.9], [0.4, 0.4, 0.05]]


def dress(seed, nu=100, nv=51):
    """(sim verts, NOCS verts, faces): a tube about the z axis whose radius waves with the angle and the height, open at both ends"""
    import numpy as np
    rng = np.random.default_rng(seed)
    a, h = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.linspace(0.0, 1.0, nv), indexing="ij")
    k, phase = rng.integers(3, 9), rng.random() * 6.28
    radius = 0.25 + 0.1 * h + 0.05 * h * np.sin(k * a + phase)
    nocs = np.stack([0.5 + radius * np.cos(a), 0.5 + radius * np.sin(a), 1.0 - 0.95 * h], axis=-1).reshape(-1, 3).astype(np.float32)
    sim = ((nocs - np.float32(0.5)) * np.float32([0.7, 0.7, 0.9]) + np.float32([0.0, 0.0, -0.43])).astype(np.float32)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv - 1), indexing="ij")
    q = np.stack([i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + j + 1, i * nv + j + 1], axis=-1).reshape(-1, 4)
    return sim, nocs, np.ascontiguousarray(np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]]), dtype=np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="profiles/point_cloud_time.json")
    ap.add_argument("--garments", type=int, default=4)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch

    from garmentnets_amd import ops, point_cloud as PC
    dev = torch.device("cuda", 0)
    meshes = [dress(s) for s in range(a.garments)]
    cams = PC.camera_ring(np.array(AABB), a.views, a.size)
    verts = torch.from_numpy(np.concatenate([m[0] for m in meshes])).to(dev)
    nocs = torch.from_numpy(np.concatenate([m[1] for m in meshes])).to(dev)
    faces = torch.from_numpy(np.concatenate([m[2] for m in meshes])).to(dev)
    vseg, fseg = np.cumsum([0] + [len(m[0]) for m in meshes]), np.cumsum([0] + [len(m[2]) for m in meshes])
    mesh_of, every = np.repeat(np.arange(a.garments), a.views), cams * a.garments

    def launch_set():
        idx = ops.depth_render_batch(verts, faces, vseg, fseg, mesh_of, every, a.size)
        return ops.depth_cloud(idx, verts, nocs, faces, vseg, fseg, mesh_of, every)

    for _ in range(a.warmup):
        launch_set()
    ms = []
    for _ in range(a.runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        point, label, rgb, sizes = launch_set()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    out = {"device_name": torch.cuda.get_device_name(0), "garments": a.garments, "views": a.views, "img_size": a.size,
           "verts_per_garment": len(meshes[0][0]), "faces_per_garment": len(meshes[0][2]), "warmup": a.warmup, "runs": a.runs,
           "interval": "events around one depth_render_batch + depth_cloud launch set (the sizes' read-back included)",
           "ms": ms, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
           "points_per_view": np.asarray(sizes).reshape(a.garments, a.views).tolist(), "points": int(np.sum(sizes))}
    if not a.no_check:
        t = time.perf_counter()
        want = PC.render_point_clouds(meshes, cams, a.size, backend="numpy")
        out["numpy_seconds"] = time.perf_counter() - t
        got = [point.cpu().numpy(), label.cpu().numpy(), rgb.cpu().numpy()]
        out["equal_numpy"] = bool(np.array_equal(np.concatenate([w["sizes"] for w in want]), sizes)) and all(
            np.array_equal(g, np.concatenate([w[k] for w in want])) for g, k in zip(got, ("point", "nocs", "rgb")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "ms"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
