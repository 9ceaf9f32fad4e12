"""What the decoder dispatch tests share (test_gpu_decoder_dispatch.py, test_decoder_dispatch_host.py, golden/make_golden_decoder_dispatch.py): the
sources, decoders, calls and arithmetics, a record of the library calls of ImplicitWNFDecoder's entries (unet_dispatch_cases.Recorder, grouped per
run_on / forward / decode_lattice), and a CPU walk of the same cases through decode_plan.  A plain module, imported by its siblings; it holds no test.

The golden (golden/decoder_dispatch_trace.json) is the launch sequence of the decoder as it stood BEFORE decode_plan existed: a refactor of the host
code of ImplicitWNFDecoder must issue the same calls with the same scalar arguments and give the same bits."""
import functools
import hashlib
import json
import os

import torch

from garmentnets_amd import ops, synthetic as S
from garmentnets_amd.arith import Arith
from garmentnets_amd.components.unet3d import FinalConv1x1
from garmentnets_amd.networks import conv_implicit_wnf as W
from unet_dispatch_cases import Recorder, _sha

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_dispatch_trace.json")

# the smallest shapes at which each branch is still taken.  folded: a UNetResult over a non-cubic pre-final volume [2][8][6][10][32] and a 32 -> 128 final
# convolution; tensor: the decoder's own entries on a (2, 128, 6, 5, 7) volume.  Garment 1 of either is 1e-8 of garment 0: the device flags it unsafe
# for fp16 planes and the gated fp32 twin computes its rows
SOURCES = {"folded": (8, 6, 10, 32), "tensor": (6, 5, 7, 128)}
B = 2
UNSAFE_SCALE = 1e-8

# shipped scalar / 3-vector decoders (the lattice brick takes the first), the class default width (no lattice form, no pack on 128 channels), and a
# width no fused kernel takes (not foldable: the materialised volume and the per-layer MLP)
DECODERS = {"256x1": (128, 256, 256, 1), "256x3": (128, 256, 256, 3), "512x1": (128, 512, 512, 1), "64x1": (128, 64, 64, 1)}

# Q = 10: the largest axis of the folded volume (the brick path); Q = 9: coarser than it, three slabs of 243 rows under a 250-row budget; the batched
# query launches, the garment loop in their place, one garment, one row, and chunks of 32, 32 and 6 rows (with the garment loop forced too: a batch
# that fits the batched launches is never chunked)
CALLS = {
    "lattice10": dict(Q=10),
    "lattice9_chunk250": dict(Q=9, ROWS_PER_CHUNK=250),
    "queries": dict(M=70),
    "queries_looped": dict(M=70, BATCH_ROWS_BYTES=0),
    "queries_b1": dict(M=70, select=(0, 1)),
    "queries_m1": dict(M=1),
    "queries_chunk32": dict(M=70, ROWS_PER_CHUNK=32),
    "queries_looped_chunk32": dict(M=70, ROWS_PER_CHUNK=32, BATCH_ROWS_BYTES=0),
}

ARITHS = {
    "default": {},
    "fp32": dict(decode_mode="fp32"),
    "no_fused_lattice": dict(fused_lattice=False),
    "no_fold_final_conv": dict(fold_final_conv=False),
}

GROUPS = ((W.ImplicitWNFDecoder, ("run_on", "forward", "decode_lattice")),)
PACKERS = ("pack_decode_split",)
REPEATS = 2                                      # calls per source: the second reads the source's caches (scales, statistics, the materialised volume)


def arith(name):
    return Arith(**ARITHS[name])


def _loaded(module, key):
    module.load_state_dict({k: S.synthetic_tensor(key + k, tuple(v.shape), 11) for k, v in module.state_dict().items()})
    return module.eval().requires_grad_(False)


@functools.lru_cache(maxsize=None)
def decoder(name, dev):
    return _loaded(W.ImplicitWNFDecoder(DECODERS[name]), f"decoder_dispatch.{name}.").to(dev)


@functools.lru_cache(maxsize=None)
def final_conv(dev):
    return _loaded(FinalConv1x1(32, 128, 1), "decoder_dispatch.final_conv.").to(dev)


def source(name, dev, select=None):
    """a fresh source (its scale / statistics caches empty): a UNetResult, or a (B, C, D, H, W) view of a channel-last volume"""
    D, H, Wd, C = SOURCES[name]
    vol = torch.relu(torch.randn(B, D, H, Wd, C, generator=torch.Generator().manual_seed(D * H + C)))     # ReLU outputs, like the pre-final volume
    vol[1] *= UNSAFE_SCALE
    vol = vol.to(dev)
    if name == "folded":
        res = W.UNetResult(vol, final_conv(dev))
        return res if select is None else res.select(*select)
    vol = vol.permute(0, 4, 1, 2, 3)
    return vol if select is None else vol[select[0]:select[1]]


def queries(M, rows, dev):
    q = torch.rand(rows, M, 3, generator=torch.Generator().manual_seed(M))
    q[:, 0] = 1.0                                # a query on the border
    return q.to(dev)


def run_call(dec, src, call, ar):
    """one call of CALLS on the source, its instance overrides set for the duration"""
    c = CALLS[call]
    dev = next(dec.parameters()).device
    over = [k for k in ("ROWS_PER_CHUNK", "BATCH_ROWS_BYTES") if k in c]
    for k in over:
        setattr(dec, k, c[k])
    try:
        rows = len(range(*c["select"])) if "select" in c else B
        q = None if "Q" in c else queries(c["M"], rows, dev)
        if isinstance(src, W.UNetResult):
            return dec.run_on(src, q, Q=c.get("Q", 0), arith=ar)
        return dec.decode_lattice(src, c["Q"], ar) if q is None else dec(src, q, ar)
    finally:
        for k in over:
            delattr(dec, k)


def record(src_name, dec_name, call, arith_name, dev="cuda:0"):
    """one call under one arithmetic, REPEATS times on one fresh source, all of it twice -> (first record, second record); a record is
    dict(trace, scalars, out, pack_builds): the entries per call of the decoder, the hash of every library call's scalar arguments, the hash of the
    outputs, the split-operand packs built (the second record's is what the golden keeps: a pack is built once per parameter state, never per call)"""
    dec, ar = decoder(dec_name, dev), arith(arith_name)
    out = []
    for _ in range(2):
        src = source(src_name, dev, CALLS[call].get("select"))
        with Recorder(groups=GROUPS, packers=PACKERS) as rec:
            ys = [run_call(dec, src, call, ar) for _ in range(REPEATS)]
        torch.cuda.synchronize()
        out.append(dict(trace=rec.trace, scalars=hashlib.sha256(json.dumps(rec.scalars).encode()).hexdigest(), out=_sha(*ys), pack_builds=rec.pack_builds))
    return out


def unsafe_flags(src_name, dec_name, dev="cuda:0"):
    """the device's verdict per garment (the third column of ops.decoder_input_scale) in one lattice call at the default arithmetic; None when no
    split-operand kernel runs there"""
    seen, orig = [], ops.decoder_input_scale

    def spy(*args):
        xs = orig(*args)
        seen.append(xs[:, 2].tolist())
        return xs
    ops.decoder_input_scale = spy
    try:
        run_call(decoder(dec_name, dev), source(src_name, dev), "lattice10", arith("default"))
    finally:
        ops.decoder_input_scale = orig
    return seen[0] if seen else None


def load_golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    for per_arith in g["cases"].values():
        for r in per_arith.values():
            r["trace"] = g["traces"][r["trace"]]
    return g


def case_id(src_name, dec_name, call):
    return f"{src_name}/{dec_name}/{call}"


def calls_of(trace):
    """a record's trace as one entry list per call of the decoder (a statistics pass noted in front of a call put back at its head)"""
    calls, front = [], []
    for t in trace:
        if isinstance(t, list):
            calls.append(front + t)
            front = []
        else:
            front.append(t)
    assert not front
    return calls


# ---------------------------------------------------------------------------------------------------- the same walk on the CPU, through decode_plan
@functools.lru_cache(maxsize=None)
def host_facts(dec_name, folded):
    """the facts of the decoder's pack (folded: on the pre-final volume), built on the CPU -- no tensor on a device, the library not loaded"""
    dec = decoder(dec_name, "cpu")
    pack = dec.folded_pack(final_conv("cpu")) if folded else dec.packed()
    return None if pack is None else pack.facts()


def plan_walk(src_name, dec_name, call, arith_name):
    """-> (plan, on_pre, B, M): the decode_plan of the case from shapes and widths alone, whether it reads the pre-final volume through a folded
    pack, the garments and the rows per garment.  Mirrors ImplicitWNFDecoder.run_on / forward / decode_lattice"""
    c, ar = CALLS[call], arith(arith_name)
    facts = host_facts(dec_name, True) if src_name == "folded" and ar.fold_final_conv else None
    on_pre = facts is not None
    if not on_pre:
        facts = host_facts(dec_name, False)
    rows = len(range(*c["select"])) if "select" in c else B
    Q = c.get("Q")
    M = c["M"] if Q is None else Q ** 3
    plan = W.decode_plan(ar, True, facts, SOURCES[src_name][:3], True, Q, rows, M, c.get("ROWS_PER_CHUNK", W.ImplicitWNFDecoder.ROWS_PER_CHUNK),
                         c.get("BATCH_ROWS_BYTES", W.ImplicitWNFDecoder.BATCH_ROWS_BYTES), True)
    return plan, on_pre, rows, M


def expected_calls(src_name, dec_name, call, arith_name):
    """the library entries of each of the REPEATS calls, expanded from plan_walk's plan"""
    plan, on_pre, rows, M = plan_walk(src_name, dec_name, call, arith_name)
    twin = ["gn_implicit_decode"] if plan.scales else []
    if plan.path == W.BATCHED:
        launches = ["gn_trilinear_sample_batch", "gn_implicit_decode_split_batch", "gn_implicit_decode_batch"]
    elif plan.path == W.LATTICE:
        launches = (["gn_implicit_decode_lattice_split"] + twin) * rows
    else:
        decode = {W.SPLIT: ["gn_implicit_decode_split"] + twin, W.FUSED: ["gn_implicit_decode"], W.MLP_LAYERS: ["gn_linear"] * 3}[plan.path]
        launches = (["gn_trilinear_sample"] + decode) * -(-M // plan.chunk) * rows
    # the first call materialises the 128-channel volume when nothing is folded, and takes the volume's statistics when a split-operand kernel runs;
    # a UNetResult remembers the scales, a tensor only the statistics
    first = (["gn_linear"] if src_name == "folded" and not on_pre else []) + (["gn_channel_stats", "gn_decoder_input_scale"] if plan.scales else [])
    again = ["gn_decoder_input_scale"] if plan.scales and not on_pre else []
    return [first + launches] + [again + launches] * (REPEATS - 1)
