"""CPU: decode_plan -- the pure launch decision of networks/conv_implicit_wnf.py -- against the launch trace recorded on the GPU before it existed.

Every case of tests/decoder_dispatch_cases.py is walked from shapes and widths alone (no tensor on a device, the library not loaded); the path and
chunking the plan names must expand to exactly the entries tests/golden/decoder_dispatch_trace.json shows each call of the decoder made."""
import inspect

import pytest
import torch

import decoder_dispatch_cases as DC
from garmentnets_amd import _lib
from garmentnets_amd.networks import conv_implicit_wnf as W

GOLDEN = DC.load_golden()


@pytest.mark.parametrize("dec", list(DC.DECODERS))
@pytest.mark.parametrize("src", list(DC.SOURCES))
def test_decode_plan_expands_to_the_recorded_launches(src, dec, monkeypatch):
    def no_library(*args):
        raise AssertionError("the plan reached for the library")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    for call in DC.CALLS:
        for name in DC.ARITHS:
            recorded = DC.calls_of(GOLDEN["cases"][DC.case_id(src, dec, call)][name]["trace"])
            assert DC.expected_calls(src, dec, call, name) == recorded, f"{DC.case_id(src, dec, call)}/{name}: {DC.plan_walk(src, dec, call, name)[0]}"


def test_the_cases_reach_every_path_and_chunking():
    """what the cases were chosen for, read off the plans: every path, one and several chunks of queries, whole lattice slabs per chunk"""
    plans = {(s, d, c, a): DC.plan_walk(s, d, c, a)[0] for s in DC.SOURCES for d in DC.DECODERS for c in DC.CALLS for a in DC.ARITHS}
    assert {p.path for p in plans.values()} == {W.LATTICE, W.BATCHED, W.SPLIT, W.FUSED, W.MLP_LAYERS}
    assert plans["folded", "256x1", "lattice10", "default"].path == W.LATTICE
    assert plans["folded", "256x1", "lattice10", "no_fused_lattice"].path == plans["folded", "256x1", "lattice9_chunk250", "default"].path == W.SPLIT
    assert plans["folded", "256x3", "lattice10", "default"].path == plans["folded", "512x1", "lattice10", "default"].path == W.SPLIT
    for (s, d, c, a), p in plans.items():
        if c == "lattice9_chunk250":
            assert p.chunk == 243, (s, d, c, a)
        if c == "queries_looped_chunk32":
            assert p.chunk == 32 and p.path != W.BATCHED, (s, d, c, a)
        assert p.scales == (p.path in (W.LATTICE, W.BATCHED, W.SPLIT)), (s, d, c, a)
    assert plans["folded", "256x1", "queries", "default"].path == plans["folded", "512x1", "queries_chunk32", "default"].path == W.BATCHED
    assert plans["folded", "256x1", "queries_looped", "default"].path == plans["folded", "256x1", "queries_b1", "default"].path == W.SPLIT


def test_decode_plan_is_pure():
    """no tensor among its arguments, and a repeated call is a cache hit"""
    names = list(inspect.signature(W.decode_plan).parameters)
    assert names == ["arith", "fused", "pack", "dims", "contiguous", "Q", "B", "M", "chunk_rows", "batch_bytes", "out_packed"]
    facts = (True, 32, 256, 1)                   # DecoderPack.facts() of the folded scalar decoder
    args = (DC.arith("default"), True, facts, (8, 6, 10), True, 10, 2, 1000, 1 << 20, 192 << 20, True)
    assert not any(isinstance(a, torch.Tensor) for a in args + tuple(facts))
    first = W.decode_plan(*args)
    hits = W.decode_plan.cache_info().hits
    assert W.decode_plan(*args) is first and W.decode_plan.cache_info().hits == hits + 1
    # `fused` off, or no pack: the per-layer MLP whatever the arithmetic
    assert W.decode_plan(args[0], False, *args[2:]).path == W.decode_plan(args[0], True, None, *args[3:]).path == W.MLP_LAYERS
