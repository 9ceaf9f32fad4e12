#!/usr/bin/env python3
"""What the f16x2 backward of the UNet convolutions costs against the fp32 one (DESIGN.md "f16x2 backward of the UNet convolutions";
profiles/unet_grad_split_time.json).

Kernel against kernel, in one process, for the two shapes DESIGN.md "UNet gradients" reports:

  training  every 3x3x3 layer of the reference's second-stage UNet (128 in, f_maps 32, 4 levels) at 32^3, B = 24, summed over the 14 layers of one
            backward pass
  single    the one 128 -> 128 layer at 128^3, B = 2

and per layer four pairs: the weight gradient (ops.conv3d_bwd_weight / ops.conv3d_bwd_weight_split, both handed y and dy), the data gradient
(ops.conv3d_bwd_data / ops.conv3d_bwd_data_split on the same masked gradient) and the masking pass in front of them (ops.relu_mask /
ops.relu_mask_max).  Alternating A B A B: 2 warm-up launches of each, then the median of 5 launches of each, every launch between two events on the
stream; min .. max recorded.  "faster": the f16x2 median is below the fp32 median by more than the larger of the two spreads (max - min).

Whole step: tools/pipeline_step_time.py's step (batch 24, 6000 points, grid 32, device packs) without and with conv_grad_mode = "f16x2", alternating.

The measurement runs in a child process under a time limit of its own (--timeout seconds).  Prints one JSON object and writes it to --out.  Not a test
and not read by bench.py.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def unet_layers(in_channels, f_maps, levels, grid):
    """(name, stored C0, stored C1, stored Cout, (D, H, W)) of every 3x3x3 layer of Abstract3DUNet(in_channels, ., f_maps, num_levels=levels)"""
    from garmentnets_amd.components.unet3d import Abstract3DUNet, stored_channels
    model = Abstract3DUNet(in_channels, in_channels, f_maps=f_maps, num_levels=levels)
    out = []
    for i, enc in enumerate(model.encoders):
        for k, sc in enumerate((enc.basic_module.SingleConv1, enc.basic_module.SingleConv2)):
            out.append((f"encoders.{i}.SingleConv{k + 1}", stored_channels(sc.conv.in_channels), 0, stored_channels(sc.conv.out_channels), (grid >> i,) * 3))
    for j, dec in enumerate(model.decoders):
        n = grid >> (levels - 2 - j)
        c1, c2 = dec.basic_module.SingleConv1, dec.basic_module.SingleConv2
        out.append((f"decoders.{j}.SingleConv1", stored_channels(c1.in_real[0]), stored_channels(c1.in_real[1]), stored_channels(c1.conv.out_channels), (n,) * 3))
        out.append((f"decoders.{j}.SingleConv2", stored_channels(c2.conv.in_channels), 0, stored_channels(c2.conv.out_channels), (n,) * 3))
    return out


def alternate(ways, warmup, runs):
    """{name: launch} -> {name: [seconds]}: all ways in turn, warmup + runs times, each launch between two stream events"""
    import torch
    times = {k: [] for k in ways}
    for i in range(warmup + runs):
        for k, launch in ways.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            launch()
            t1.record()
            t1.synchronize()
            if i >= warmup:
                times[k].append(t0.elapsed_time(t1) * 1e-3)
    return times


def stat(t):
    return {"ms": [v * 1e3 for v in t], "ms_median": statistics.median(t) * 1e3, "ms_min": min(t) * 1e3, "ms_max": max(t) * 1e3}


def faster(fp32, split):
    spread = max(fp32["ms_max"] - fp32["ms_min"], split["ms_max"] - split["ms_min"])
    return bool(fp32["ms_median"] - split["ms_median"] > spread)


def time_layer(name, c0, c1, cout, dims, B, a):
    import torch

    from garmentnets_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(c0 + c1 + cout + dims[0])
    src0 = torch.randn((B, *dims, c0), generator=g, device=dev)
    src1 = torch.randn((B, *(n // 2 for n in dims), c1), generator=g, device=dev) if c1 else None
    y = torch.randn((B, *dims, cout), generator=g, device=dev)
    dy = torch.randn((B, *dims, cout), generator=g, device=dev)
    w = torch.randn((cout, c0 + c1, 3, 3, 3), generator=g, device=dev) * 0.05
    gamma, beta = torch.ones(c0 + c1, device=dev), torch.zeros(c0 + c1, device=dev)
    st0 = ops.channel_stats(src0)
    st1 = None if src1 is None else ops.channel_stats(src1)
    aa, dd = ops.groupnorm_affine(st0, st1, 8, 1e-5, gamma, beta)
    a_s, d_s, x_inv = ops.groupnorm_affine(st0, st1, 8, 1e-5, gamma, beta, with_act_scale=True)
    gm, gmax, scale, inv = ops.relu_mask_max(y, dy)
    cin_p = -(-(c0 + c1) // 32) * 32
    wpt = ops.pack_conv_weight_bwd_data(w)
    pack = ops.pack_conv_weight_bwd_data_split(w, True)
    ways = {"weight_fp32": lambda: ops.conv3d_bwd_weight(src0, src1, aa, dd, y, dy),
            "weight_f16x2": lambda: ops.conv3d_bwd_weight_split(src0, src1, a_s, d_s, y, dy, x_inv=x_inv, gmax=gmax),
            "data_fp32": lambda: ops.conv3d_bwd_data(gm, wpt, cin_p),
            "data_f16x2": lambda: ops.conv3d_bwd_data_split(gm, scale, inv, pack, cin_p),
            "mask_fp32": lambda: ops.relu_mask(y, dy),
            "mask_f16x2": lambda: ops.relu_mask_max(y, dy)}
    res = {k: stat(t) for k, t in alternate(ways, a.warmup, a.runs).items()}
    out = {"layer": name, "c0": c0, "c1": c1, "cout": cout, "dims": list(dims), "B": B, **res}
    for kind in ("weight", "data", "mask"):
        out[kind + "_f16x2_faster"] = faster(res[kind + "_fp32"], res[kind + "_f16x2"])
        out[kind + "_speedup"] = res[kind + "_fp32"]["ms_median"] / res[kind + "_f16x2"]["ms_median"]
    torch.cuda.empty_cache()
    return out


def total(rows):
    """the layers of one backward pass summed: medians, mins and maxes added (the spread of the sum is at most the sum of the spreads)"""
    out = {}
    for k in ("weight_fp32", "weight_f16x2", "data_fp32", "data_f16x2", "mask_fp32", "mask_f16x2"):
        out[k] = {q: sum(r[k][q] for r in rows) for q in ("ms_median", "ms_min", "ms_max")}
    for kind in ("weight", "data", "mask"):
        out[kind + "_f16x2_faster"] = faster(out[kind + "_fp32"], out[kind + "_f16x2"])
        out[kind + "_speedup"] = out[kind + "_fp32"]["ms_median"] / out[kind + "_f16x2"]["ms_median"]
    return out


def time_step(a):
    import torch

    from garmentnets_amd import synthetic
    from garmentnets_amd.batch import Batch
    from garmentnets_amd.networks.conv_implicit_wnf import ConvImplicitWNFPipeline
    from pipeline_step_time import PARTS, timed_step
    dev = torch.device("cuda:0")
    hp = synthetic.default_hparams(grid=32, reduce_method="max")
    model = ConvImplicitWNFPipeline(**hp)
    model.load_state_dict(synthetic.synthetic_state_dict(hp, 0, planted_nocs=True))
    model = model.to(dev).requires_grad_(True).train()
    B, n = a.batch, 6000
    x, pos, b = synthetic.synthetic_cloud(B, n, seed=0, colour="position")
    g = torch.Generator().manual_seed(0)
    batch = Batch(sizes=[n] * B, x=x, pos=pos, batch=b, volume_query_points=torch.rand(B, n, 3, generator=g), gt_volume_value=torch.rand(B, n, generator=g),
                  surf_query_points=torch.rand(B, n, 3, generator=g), gt_sim_points=0.3 * torch.randn(B, n, 3, generator=g)).to(dev)
    opt = model.configure_optimizers()
    model.arith = model.arith.replace(device_packs=True)
    ariths = {"fp32": model.arith, "f16x2": model.arith.replace(conv_grad_mode="f16x2")}
    rows = {k: [] for k in ariths}
    for i in range(a.step_warmup + a.steps):
        for k, arith in ariths.items():
            t = timed_step(model, opt, batch, arith)
            if i >= a.step_warmup:
                rows[k].append(t)
    out = {"batch": B, "points": n, "queries": n, "grid": 32, "device_packs": True, "steps": a.steps, "warmup": a.step_warmup, "order": "fp32, f16x2, fp32, f16x2, ..."}
    for k, r in rows.items():
        # (bracketed() gives milliseconds, stat() takes seconds)
        out[k] = {"step": stat([sum(t) * 1e-3 for t in r]), "backward": stat([t[PARTS.index("backward")] * 1e-3 for t in r])}
    out["step_f16x2_faster"] = faster(out["fp32"]["step"], out["f16x2"]["step"])
    return out


def measure(a):
    import torch
    out = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "runs": a.runs, "order": "fp32, f16x2, fp32, f16x2, ... per pair"}
    if "training" in a.what:
        rows = [time_layer(*layer, a.batch, a) for layer in unet_layers(128, 32, 4, 32)]
        out["training"] = {"shape": "in 128, f_maps 32, 4 levels, 32^3, B = %d" % a.batch, "layers": rows, "per_backward_pass": total(rows)}
    if "single" in a.what:
        out["single"] = time_layer("128 -> 128 at 128^3", 128, 0, 128, (128, 128, 128), 2, a)
    if "step" in a.what:
        out["step"] = time_step(a)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="profiles/unet_grad_split_time.json")
    ap.add_argument("--what", default="training,single,step", help="comma-separated: training, single, step")
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--step_warmup", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=540.0, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.what = a.what.split(",")
    if a.child:
        print(json.dumps(measure(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--what", ",".join(a.what), "--batch", str(a.batch), "--warmup", str(a.warmup), "--runs",
           str(a.runs), "--steps", str(a.steps), "--step_warmup", str(a.step_warmup)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
    if res.returncode != 0:
        return res.returncode
    out = json.loads(res.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    print(json.dumps({k: (v if not isinstance(v, dict) else {q: v[q] for q in v if q != "layers"}) for k, v in out.items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
