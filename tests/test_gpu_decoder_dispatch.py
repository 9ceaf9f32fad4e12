"""GPU (-m gpu): the implicit decoder launches what it launched before decode_plan existed.

tests/golden/decoder_dispatch_trace.json was recorded at the parent of the change that introduced decode_plan (golden/make_golden_decoder_dispatch.py):
per source, decoder, call and arithmetic of tests/decoder_dispatch_cases.py the library entries of every call of the decoder, a hash of every library
call's scalar arguments, the hash of the outputs, and the number of split-operand packs built by a second run on the same decoder.  The same cases run
through the present code must reproduce all four: a refactor of the host code issues the same launches and gives the same bits."""
import pytest

pytestmark = pytest.mark.gpu

import decoder_dispatch_cases as DC  # noqa: E402

GOLDEN = DC.load_golden()


@pytest.mark.parametrize("dec", list(DC.DECODERS))
@pytest.mark.parametrize("src", list(DC.SOURCES))
def test_decoder_dispatch_reproduces_the_recorded_launches(src, dec):
    for call in DC.CALLS:
        for name in DC.ARITHS:
            where = f"{DC.case_id(src, dec, call)}/{name}"
            want = GOLDEN["cases"][DC.case_id(src, dec, call)][name]
            first, second = DC.record(src, dec, call, name)
            for got in (first, second):
                assert got["trace"] == want["trace"], f"{where}: launches differ"
                assert got["scalars"] == want["scalars"], f"{where}: scalar arguments differ"
                assert got["out"] == want["out"], f"{where}: same launches, other bits"
            assert second["pack_builds"] == want["pack_builds"] == 0, f"{where}: a pack was rebuilt on a second call"


def test_the_decoder_hands_decode_plan_no_tensor(monkeypatch):
    import torch
    seen, plan = [], DC.W.decode_plan

    def spy(*args):
        seen.append(args)
        return plan(*args)
    monkeypatch.setattr(DC.W, "decode_plan", spy)
    for src in DC.SOURCES:
        for call in ("lattice10", "queries"):
            DC.run_call(DC.decoder("256x1", "cuda:0"), DC.source(src, "cuda:0"), call, DC.arith("default"))
    assert len(seen) == 4
    for args in seen:
        assert not any(isinstance(a, torch.Tensor) for a in args + tuple(args[2])), args


@pytest.mark.parametrize("src", list(DC.SOURCES))
def test_the_second_garment_is_on_the_gated_fp32_twin(src):
    """what the sources were scaled for: the device flags garment 1, and garment 1 alone, unsafe for fp16 planes"""
    assert DC.unsafe_flags(src, "256x1") == [0.0, 1.0]
