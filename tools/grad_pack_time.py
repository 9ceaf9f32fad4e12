#!/usr/bin/env python3
"""Time gn_grad_pack at the second stage's real gradient layout on one MI355X: tools/grad_pack_time.py [--out profiles/grad_pack_time.json]

The layout is the one parallel.GradientReducer forms for ConvImplicitWNFPipeline(**synthetic.default_hparams()): every parameter outside the frozen first
stage, in the optimiser's order, each gradient a tensor of its own (as backward leaves them after zero_grad(set_to_none=True)), offsets from
parallel.plan_flat.  Three ways to bring them into one flat buffer, on the same tensors in the same run, each the median of 20 launches after 5, bracketed
by events on the stream:
  grad_pack      ops.grad_pack, one launch (world 2: the division is in)
  torch_cat      torch.cat([g.reshape(-1) for g in grads])
  foreach_copy   torch._foreach_copy_ into the views of the flat buffer
and the bound a pure copy has: 2 x 4 bytes per element over the card's HBM bandwidth (MI355X: 8.0 TB/s by its specification, 6.29 TB/s measured with a
float4 copy).  Not a test and not read by bench.py.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from garmentnets_amd import ops, parallel, synthetic  # noqa: E402
from garmentnets_amd.networks.conv_implicit_wnf import ConvImplicitWNFPipeline  # noqa: E402

WARMUP, LAUNCHES = 5, 20
HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12      # bytes / s


def median_ms(fn):
    times = []
    for i in range(WARMUP + LAUNCHES):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        if i >= WARMUP:
            times.append(start.elapsed_time(end))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grad_pack_time.json"))
    ap.add_argument("--world", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/grad_pack_time.py needs a GPU")
    dev = torch.device("cuda:0")
    model = ConvImplicitWNFPipeline(**synthetic.default_hparams()).to(dev)
    first = {id(p) for p in model.pointnet2_nocs.parameters()}
    params = [p for p in model.parameters() if id(p) not in first]
    g = torch.Generator(device=dev).manual_seed(0)
    grads = [torch.randn(p.shape, device=dev, generator=g) for p in params]
    numels = [t.numel() for t in grads]
    offsets, total = parallel.plan_flat(numels)
    flat = torch.zeros(total, dtype=torch.float32, device=dev)
    table, blocks = ops.grad_pack_table([(t.data_ptr(), off, n) for t, off, n in zip(grads, offsets, numels)], dev)
    views = [flat[off:off + n].view_as(t) for t, off, n in zip(grads, offsets, numels)]

    ops.grad_pack(table, len(grads), blocks, flat, 1)
    assert all(torch.equal(v, t) for v, t in zip(views, grads))                       # world 1 is the copy
    result = {"tensors": len(grads), "floats": sum(numels), "flat_floats": total, "workgroups": blocks, "world": a.world,
              "warmup": WARMUP, "launches": LAUNCHES, "device": torch.cuda.get_device_name(0)}
    for name, fn in (("grad_pack", lambda: ops.grad_pack(table, len(grads), blocks, flat, a.world)),
                     ("torch_cat", lambda: torch.cat([t.reshape(-1) for t in grads])),
                     ("foreach_copy", lambda: torch._foreach_copy_(views, grads))):
        med, lo, hi = median_ms(fn)
        result[name] = {"median_ms": med, "min_ms": lo, "max_ms": hi}
    nbytes = 2 * 4 * sum(numels)
    result["bytes_moved"] = nbytes
    result["bound_ms"] = {"hbm_spec_8.0TBps": nbytes / HBM_SPEC * 1e3, "hbm_measured_6.29TBps": nbytes / HBM_MEASURED * 1e3}
    result["grad_pack_bytes_per_s"] = nbytes / (result["grad_pack"]["median_ms"] * 1e-3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=2)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
