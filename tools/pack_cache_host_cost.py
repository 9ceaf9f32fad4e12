#!/usr/bin/env python3
"""Host cost of the pack caches' generation rule (components.mlp.generation): tools/pack_cache_host_cost.py [--counts FILE.json] [--ms-per-step MS]

Times one generation() per module type of the benchmark's model on the CPU (no device is needed to construct the modules): the held-list form a
PackedModule takes, and for comparison the walk over parameters() and buffers().  With a GPU it also counts the generation computations of one
predict_batch of the benchmark's model per module type (the function wrapped in every module that imports it) and writes them to --counts; without
one it reads the counts from that file.  Prints the product, summed over a step, against 0.2 % of --ms-per-step.  Not a test and not read by bench.py."""
import argparse
import collections
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from garmentnets_amd import synthetic as S  # noqa: E402
from garmentnets_amd.batch import Batch  # noqa: E402
from garmentnets_amd.components import mlp, pointnet2, unet3d  # noqa: E402
from garmentnets_amd.networks import conv_implicit_wnf as W  # noqa: E402
from garmentnets_amd.predict import predict_batch  # noqa: E402

CONFIGS = {"ms_per_step": dict(B=16, grid=128, Q=128), "latency_b1": dict(B=1, grid=32, Q=128)}


def _model(grid):
    hp = S.default_hparams(grid=grid, reduce_method="mean")
    model = W.ConvImplicitWNFPipeline(**hp)
    model.load_state_dict(S.synthetic_state_dict(hp, 0, planted_nocs=True, planted_wnf=True))
    return model.eval().requires_grad_(False)


def count(dev="cuda:0"):
    """{config: {module type: generation computations of one warm predict_batch}}"""
    counts, orig = collections.Counter(), mlp.generation

    def counted(module, *extra, tensors=None):
        counts[type(module).__name__] += 1
        return orig(module, *extra, tensors=tensors)
    for mod in (mlp, unet3d, pointnet2, W):
        mod.generation = counted
    out = {}
    try:
        for name, c in CONFIGS.items():
            model = _model(c["grid"]).to(dev)
            x, pos, _ = S.synthetic_cloud(1, 6000, seed=4242, colour="position")
            B = c["B"]
            data = Batch(sizes=[6000] * B, x=x.repeat(B, 1), pos=pos.repeat(B, 1), batch=torch.arange(B).repeat_interleave(6000)).to(dev)
            for _ in range(2):                                  # the second, warm call is the one counted
                counts.clear()
                predict_batch(model, data, volume_size=c["Q"])
                torch.cuda.synchronize()
            out[name] = dict(counts)
    finally:
        for mod in (mlp, unet3d, pointnet2, W):
            mod.generation = orig
    return out


def times(reps=20000):
    """{module type: (tensors, us per held-list generation, us per walk)} over the benchmark's model, the largest module of each type"""
    best = {}
    for m in _model(128).modules():
        if isinstance(m, mlp.PackedModule):
            n = len(list(m.parameters())) + len(list(m.buffers()))
            if n > best.get(type(m).__name__, (None, -1))[1]:
                best[type(m).__name__] = (m, n)
    out = {}
    for name, (m, n) in sorted(best.items()):
        mlp.generation(m)
        t0 = time.perf_counter()
        for _ in range(reps):
            mlp.generation(m)
        held = (time.perf_counter() - t0) / reps * 1e6
        t0 = time.perf_counter()
        for _ in range(reps // 20):
            tuple(t._version for t in list(m.parameters()) + list(m.buffers()))
        out[name] = (n, held, (time.perf_counter() - t0) / (reps // 20) * 1e6)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--counts", default=None, help="JSON file of the counts: written when a GPU is present, read otherwise")
    ap.add_argument("--ms-per-step", type=float, default=None, help="the benchmark's ms_per_step the bound is 0.2 %% of")
    a = ap.parse_args()
    if torch.cuda.is_available():
        counts = count()
        if a.counts:
            with open(a.counts, "w") as f:
                json.dump(counts, f, indent=1)
    elif a.counts and os.path.exists(a.counts):
        counts = json.load(open(a.counts))
    else:
        counts = None
    t = times()
    print("generation() per call, CPU (tensors, held list us, walk of parameters() + buffers() us):")
    for name, (n, held, walk) in t.items():
        print(f"  {name:22s} {n:3d} tensors  {held:6.2f} us  {walk:7.2f} us")
    for cfg, per_type in (counts or {}).items():
        total = sum(per_type.values())
        us = sum(k * t.get(name, max(t.values(), key=lambda v: v[1]))[1] for name, k in per_type.items())
        print(f"one predict_batch ({cfg}: {CONFIGS[cfg]}): {total} generation computations {per_type} -> {us / 1e3:.4f} ms of host time")
        if a.ms_per_step and cfg == "ms_per_step":
            print(f"  bound: 0.2 % of {a.ms_per_step} ms = {0.002 * a.ms_per_step:.4f} ms -> {'within' if us / 1e3 < 0.002 * a.ms_per_step else 'OVER'}")


if __name__ == "__main__":
    main()
