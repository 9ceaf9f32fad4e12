"""GPU (-m gpu): the UNet's training path launches what it launched before the weight packs were keyed by one generation rule, and follows an
in-place parameter update.

tests/golden/unet_grad_dispatch_trace.json was recorded at the parent of that change (golden/make_golden_unet_grad_dispatch.py): per case and arithmetic
of tests/unet_grad_dispatch_cases.py the library entries of autograd.unet3d's forward and backward, a hash of every call's scalar arguments, the hashes
of the output and of every gradient, and the number of weight packs each of two runs of one model built.  The present code must reproduce all of it.
Then, against a fresh copy and not against the golden: after every parameter is multiplied in place by 1.01 a third run builds exactly the packs the
first one built and gives the bits of a deepcopy of the updated model run once (under conv_mode fp32 the parent served the old fp32 pack here)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import unet_grad_dispatch_cases as GC  # noqa: E402

GOLDEN = GC.load_golden()


@pytest.mark.parametrize("name", list(GC.ARITHS))
@pytest.mark.parametrize("case", list(GC.CASES))
def test_unet_grad_dispatch_reproduces_the_recorded_launches(case, name):
    want = GOLDEN["cases"][case][name]
    net, x, gy, ar, (first, second) = GC.record(case, name)
    for got in (first, second):
        assert got["trace"] == want["trace"], f"{case}/{name}: launches differ"
        assert got["scalars"] == want["scalars"], f"{case}/{name}: scalar arguments differ"
        assert got["out"] == want.get("out", got["out"]), f"{case}/{name}: same launches, other output bits"
        assert set(got["grads"]) >= set(want["grads"])
        for n, h in want["grads"].items():
            assert got["grads"][n] == h, f"{case}/{name}: same launches, other bits in the gradient of {n}"
    assert [first["pack_builds"], second["pack_builds"]] == want["pack_builds"] and second["pack_builds"] == 0, f"{case}/{name}: pack builds"
    assert first["pack_scalars"] == want["pack_scalars"], f"{case}/{name}: the device builders' launches differ"

    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.01)
    third = GC.run_once(net, x, gy, ar)
    fresh = GC.run_once(copy.deepcopy(net), x, gy, ar)
    assert third["pack_builds"] == first["pack_builds"] == fresh["pack_builds"], f"{case}/{name}: packs built after an in-place update"
    assert third["pack_scalars"] == first["pack_scalars"]
    assert third["trace"] == want["trace"] and third["scalars"] == want["scalars"]
    assert third["out"] != first["out"], f"{case}/{name}: the update did not reach the output"
    assert third["out"] == fresh["out"], f"{case}/{name}: a stale pack after an in-place update"
    for n, h in fresh["grads"].items():
        assert third["grads"][n] == h, f"{case}/{name}: a stale pack after an in-place update (gradient of {n})"
