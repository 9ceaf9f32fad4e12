"""What the UNet gradient dispatch tests share (test_gpu_unet_grad_dispatch.py, golden/make_golden_unet_grad_dispatch.py): the cases, the arithmetics
and one recorded training pass -- autograd.unet3d forward plus torch.autograd.grad -- of a model.  A plain module, imported by its siblings; it holds no
test.

The golden (golden/unet_grad_dispatch_trace.json) is the launch sequence of the training path as it stood BEFORE the weight packs were keyed by one
generation rule: a refactor of the host code behind the packs and behind _ConvGcr.backward must issue the same calls with the same scalar arguments,
give the same bits and build every pack once."""
import hashlib
import json
import os

import torch

from garmentnets_amd import autograd as A, synthetic as S
from garmentnets_amd.arith import CONV_FP32, Arith
from garmentnets_amd.components import unet3d as U

import unet_dispatch_cases as DC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_grad_dispatch_trace.json")

# the two smallest models that reach every branch of the backward.  "padded": channel-padded storage (24 / 48 / 96 / 192 real channels), decoders with
# two padded sources, the pad slices of the weight gradient.  "unpadded": no layout at all -- the forward's fp32 pack is SingleConv.packed()'s
CASES = {
    "padded": dict(in_channels=32, f_maps=24, num_levels=4, grid=16, B=2),
    "unpadded": dict(in_channels=32, f_maps=32, num_levels=3, grid=16, B=2),
}

ARITHS = {
    "default": {},
    "f16x2": dict(conv_grad_mode="f16x2"),
    "f16x2_device_packs": dict(conv_grad_mode="f16x2", device_packs=True),
    "fp32": dict(conv_mode=CONV_FP32),
}

# the forward's host builders, the backward's and the device builders
PACKERS = DC.PACKERS + ("pack_conv_weight_bwd_data", "pack_conv_weight_bwd_data_split", "pack_conv_weight_split_device",
                        "pack_conv_weight_split_wino_device", "pack_upconv_weight_device")


def arith(name):
    return Arith(**ARITHS[name])


def model(case):
    c = CASES[case]
    net = U.Abstract3DUNet(in_channels=c["in_channels"], out_channels=16, f_maps=c["f_maps"], num_levels=c["num_levels"])
    net.load_state_dict({k: S.synthetic_tensor("grad_dispatch." + k, tuple(v.shape), 11) for k, v in net.state_dict().items()})
    return net.eval()


def inputs(case, dev):
    """-> (x (B, C, G, G, G), the gradient at the output (B, 16, G, G, G)), seeded"""
    c = CASES[case]
    g = torch.Generator().manual_seed(2000 + c["f_maps"])
    x = torch.randn(c["B"], c["in_channels"], c["grid"], c["grid"], c["grid"], generator=g)
    gy = torch.randn(c["B"], 16, c["grid"], c["grid"], c["grid"], generator=g)
    return x.to(dev), gy.to(dev)


def _digest(calls):
    return hashlib.sha256(json.dumps(calls).encode()).hexdigest()


def run_once(net, x, gy, ar):
    """one training pass under the recorder -> dict(trace, scalars, pack_scalars, out, grads, pack_builds): the flat sequence of library entries
    (forward, then backward), the hash of every call's scalar arguments, the same of the device builders' own launches (gn_weight_pack_*: kept apart,
    a run that finds its packs cached has none), the hash of the output, {name: hash} of the gradient at x and at every parameter, and the number of
    weight packs built.  The weight-gradient entries do not note the kernel they launch: gn_last_kernel() after them names an earlier launch of the
    calling thread -- autograd's, so one of the PREVIOUS backward -- and is dropped."""
    names = [n for n, _ in net.named_parameters()]
    xr = x.detach().clone().requires_grad_(True)
    with DC.Recorder(groups=(), packers=PACKERS) as rec:
        y = A.unet3d(net, xr, arith=ar)
        grads = torch.autograd.grad(y, [xr] + list(net.parameters()), gy)
    torch.cuda.synchronize()
    trace = [t.split(":")[0] if t.startswith("gn_conv3d_bwd_weight") else t for t in rec.trace if not t.startswith("gn_weight_pack_")]
    return dict(trace=trace, scalars=_digest([c for c in rec.scalars if not c[0].startswith("gn_weight_pack_")]),
                pack_scalars=_digest([c for c in rec.scalars if c[0].startswith("gn_weight_pack_")]), out=DC._sha(y),
                grads={n: DC._sha(g) for n, g in zip(["x"] + names, grads)}, pack_builds=rec.pack_builds)


def record(case, arith_name, dev="cuda:0"):
    """one case under one arithmetic, run twice on the same model -> (the model, x, gy, the arithmetic, [first run's record, second run's])"""
    net, ar = model(case).to(dev), arith(arith_name)
    x, gy = inputs(case, dev)
    return net, x, gy, ar, [run_once(net, x, gy, ar) for _ in range(2)]


def load_golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    for per_arith in g["cases"].values():
        for r in per_arith.values():
            r["trace"] = g["traces"][r["trace"]]
    return g
