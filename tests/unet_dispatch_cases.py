"""What the UNet dispatch tests share (test_gpu_unet_dispatch.py, test_unet_dispatch_host.py, golden/make_golden_unet_dispatch.py): the cases, the
arithmetics, a recorder of the library calls of one Abstract3DUNet.run, and a CPU walk of the same model through conv_plan.  A plain module,
imported by its siblings; it holds no test.

The golden (golden/unet_dispatch_trace.json) is the launch sequence of the dispatch as it stood BEFORE conv_plan existed: a refactor of the host
code behind SingleConv must issue the same calls with the same scalar arguments and give the same bits."""
import functools
import hashlib
import json
import os

import torch

from garmentnets_amd import _lib, ops, synthetic as S
from garmentnets_amd.arith import CONV_FP32, SPLIT_BF16X3, Arith
from garmentnets_amd.components import unet3d as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_dispatch_trace.json")

# the smallest shapes at which each branch is still taken.  A: the shipped widths -- 128-wide Winograd, affine-in-weights with and without
# Winograd, the direct kernels, polyphase on the direct kernel, the last decoder's skip at rest.  B: the 32-wide Winograd kernel (needs 64^3),
# its _partial entry, rest0 through Winograd.  C: channel-padded storage (24 / 48 / 96 / 192 real channels; the pool over 96 stored channels is
# the one whose statistics do not come from its epilogue).  "dense": the same scattered input handed over without its cells and statistics
CASES = {
    "A": dict(in_channels=128, f_maps=32, levels=4, grid=32, B=2, sparse=True),
    "A_dense": dict(in_channels=128, f_maps=32, levels=4, grid=32, B=2, sparse=False),
    "B": dict(in_channels=32, f_maps=32, levels=2, grid=64, B=1, sparse=True),
    "B_dense": dict(in_channels=32, f_maps=32, levels=2, grid=64, B=1, sparse=False),
    "C": dict(in_channels=32, f_maps=24, levels=4, grid=16, B=2, sparse=True),
}

ARITHS = {
    "default": {},
    "no_sparse_first_conv": dict(sparse_first_conv=False),
    "no_affine_in_weights": dict(affine_in_weights=False),
    "no_winograd": dict(winograd=False),
    "no_winograd32": dict(winograd32=False),
    "no_polyphase_upconv": dict(polyphase_upconv=False),
    "fp32": dict(conv_mode=CONV_FP32),
    "bf16x3": dict(conv_mode=SPLIT_BF16X3),
}

PACKERS = ("pack_conv_weight", "pack_conv_weight_split", "pack_conv_weight_split_wino", "pack_upconv_weight", "polyphase_weights")
LAYER_ENTRIES = ("run", "run_at_rest")          # SingleConv's run entries (whichever of them the class has)


def arith(name):
    return Arith(**ARITHS[name])


def model(case):
    c = CASES[case]
    net = U.Abstract3DUNet(in_channels=c["in_channels"], out_channels=16, f_maps=c["f_maps"], num_levels=c["levels"])
    net.load_state_dict({k: S.synthetic_tensor("dispatch." + k, tuple(v.shape), 7) for k, v in net.state_dict().items()})
    return net.eval().requires_grad_(False)


def scattered_input(case, dev):
    """-> (volume, statistics, flat cell index) of a seeded cloud; the last garment of a batch of more than one has no point"""
    c = CASES[case]
    G, B, C = c["grid"], c["B"], c["in_channels"]
    g = torch.Generator().manual_seed(1000 + G + C)
    flat = []
    for b in range(max(1, B - 1)):
        cells = torch.cat([torch.tensor([[0, 0, 0], [G - 1, G - 1, G - 1], [0, G - 1, 5]]), torch.randint(0, G, (150, 3), generator=g)])
        flat.append(((b * G + cells[:, 0]) * G + cells[:, 1]) * G + cells[:, 2])
    flat = torch.cat(flat).to(torch.int32).to(dev)
    feats = torch.randn(flat.numel(), C, generator=g).to(dev)
    vol, stats = ops.grid_scatter(feats, flat, B, (G, G, G), "max", with_stats=True)
    return vol, stats, flat


def _scalar(v):
    """an argument of a C-ABI call as recorded: ints and floats as they are, a pointer as null (0) / non-null (1)"""
    if v is None:
        return "p0"
    if hasattr(v, "value") and not isinstance(v, (int, float)):        # ctypes.c_void_p
        return "p1" if v.value else "p0"
    return repr(v)


class Recorder:
    """for the duration of the `with` block: every garmentnets_amd._lib.call noted as (entry, gn_last_kernel() after it, scalar arguments), grouped per
    invocation of one of `groups` -- (class, method names) pairs, by default SingleConv's run entries; the `packers` of ops counted.  A statistics pass
    at the head of a group (gn_channel_stats[_any] over its input, before anything else of the group) is noted in FRONT of the group: it belongs to
    whoever produced that input, not to the group's dispatch."""

    def __init__(self, groups=None, packers=PACKERS):
        self.groups = ((U.SingleConv, LAYER_ENTRIES),) if groups is None else groups
        self.packers = packers

    def __enter__(self):
        self.trace, self.scalars, self.pack_builds, self._group, self._saved = [], [], 0, None, []
        lib = _lib.load()
        orig_call = _lib.call

        def call(name, *args):
            rc = orig_call(name, *args)
            # (only the gn_conv3d_* entries note the kernel they launched: after any other entry gn_last_kernel() still names an earlier launch)
            item = f"{name}:{lib.gn_last_kernel().decode()}" if name.startswith("gn_conv3d_") else name
            self.scalars.append((name, [_scalar(a) for a in args]))
            if self._group is None or (not self._group and name.startswith("gn_channel_stats")):
                self.trace.append(item)
            else:
                self._group.append(item)
            return rc
        self._patch(_lib, "call", call)

        def layer(orig):
            def run(conv, *args, **kwargs):
                if self._group is not None:                            # (an entry that calls its sibling: one layer)
                    return orig(conv, *args, **kwargs)
                self._group = []
                try:
                    return orig(conv, *args, **kwargs)
                finally:
                    self.trace.append(self._group)
                    self._group = None
            return run
        for cls, names in self.groups:
            for name in names:
                if hasattr(cls, name):
                    self._patch(cls, name, layer(getattr(cls, name)))

        def counted(orig):
            def build(*args, **kwargs):
                self.pack_builds += 1
                return orig(*args, **kwargs)
            return build
        for name in self.packers:
            self._patch(ops, name, counted(getattr(ops, name)))
        return self

    def _patch(self, obj, name, value):
        self._saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def __exit__(self, *exc):
        for obj, name, value in reversed(self._saved):
            setattr(obj, name, value)
        return False


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def record(case, arith_name, dev="cuda:0"):
    """one case under one arithmetic, run twice on the same model -> (first run's record, second run's record); a record is
    dict(trace, scalars, out, stats, pack_builds).  The second run's pack_builds is what the golden keeps (a pack is built once per layer, parameter
    version and layout, never per call).  stats: the hash of the pre-final volume's sum (fp64, every bit: sums of fp32 partials are exact) and of its
    sumsq ROUNDED TO fp32: the order of the epilogues' fp64 atomics moves the last bits of that sum from run to run (measured on this path: up to
    1.7e-15 relative, the output bits equal), so its fp64 bits are no property of the code; 24 of its 53 bits are"""
    net, ar = model(case).to(dev), arith(arith_name)
    vol, stats, flat = scattered_input(case, dev)
    if not CASES[case]["sparse"]:
        stats = flat = None
    out = []
    for _ in range(2):
        with Recorder() as rec:
            pre, (s, q, _) = net.run(vol, stats, pre_final=True, return_stats=True, sparse_flat=flat, arith=ar)
        torch.cuda.synchronize()
        out.append(dict(trace=rec.trace, scalars=hashlib.sha256(json.dumps(rec.scalars).encode()).hexdigest(), out=_sha(pre), stats=_sha(s, q.float()),
                        pack_builds=rec.pack_builds))
    return out


def load_golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    for per_arith in g["cases"].values():
        for r in per_arith.values():
            r["trace"] = g["traces"][r["trace"]]
    return g


# ---------------------------------------------------------------------------------------------------- the same walk on the CPU, through conv_plan
@functools.lru_cache(maxsize=None)
def _host_model(case):
    return model(case)                             # (never moved to a device: record() builds its own)


def plan_walk(case, arith_name, B):
    """the conv_plan of every SingleConv of the case's model in launch order, from shapes and layer widths alone (no tensor on a device, the library
    not loaded).  Mirrors Abstract3DUNet.run: the first encoder behind the scatter (cells known when the case hands them over), max-pools between the
    encoders, each decoder on (skip, coarse x); the last decoder's skip at rest when the first encoder reported a rest value"""
    c, ar, net = CASES[case], arith(arith_name), _host_model(case)
    sc = U.stored_channels
    shape = (B, c["grid"], c["grid"], c["grid"], c["in_channels"])      # what a layer would be handed: only its sample dims reach the plan
    plans, skips = [], []
    for i, enc in enumerate(net.encoders):
        if i > 0:
            shape = (B,) + tuple(n // 2 for n in shape[1:4]) + shape[4:]
        dc = enc.basic_module
        reach, known, small = (1, True, None) if i == 0 and c["sparse"] else (0, False, None)
        for conv in (dc.SingleConv1, dc.SingleConv2):
            cout = sc(conv.conv.out_channels)
            p = U.conv_plan(ar, shape[1:4], shape[4], 0, cout, reach=reach, rest_known=known, small=small, cells=reach > 0)
            plans.append(p)
            if reach and (p.aiw or p.small):
                reach, known, small = reach + 1, p.aiw, (p.small,) * 3 if p.small else None
            else:
                reach, known, small = 0, False, None
            shape = shape[:4] + (cout,)
        skips.insert(0, (shape, reach > 0 and known))    # the block's output at a known rest value: the affine-in-weights form ran last
    for dec, (skip, rest0) in zip(net.decoders, skips[1:]):
        dc = dec.basic_module
        cout = sc(dc.SingleConv1.conv.out_channels)
        plans.append(U.conv_plan(ar, skip[1:4], skip[4], shape[4], cout, rest0=rest0))
        plans.append(U.conv_plan(ar, skip[1:4], cout, 0, sc(dc.SingleConv2.conv.out_channels)))
        shape = skip[:4] + (sc(dc.SingleConv2.conv.out_channels),)
    return plans
