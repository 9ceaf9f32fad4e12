"""CPU: conv_plan -- the pure launch decision of components/unet3d.py -- against the launch trace recorded on the GPU before it existed.

Every case of tests/unet_dispatch_cases.py is walked from shapes and layer widths alone (no tensor on a device, the library not loaded); per layer
the plan must say what tests/golden/unet_dispatch_trace.json shows that layer launched."""
import pytest

import unet_dispatch_cases as DC
from garmentnets_amd import _lib
from garmentnets_amd.arith import CONV_FP32

GOLDEN = DC.load_golden()


@pytest.mark.parametrize("case", list(DC.CASES))
@pytest.mark.parametrize("name", list(DC.ARITHS))
def test_conv_plan_agrees_with_the_recorded_launches(case, name, monkeypatch):
    def no_library(*args):
        raise AssertionError("the plan reached for the library")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    layers = [[item.split(":")[0] for item in t] for t in GOLDEN["cases"][case][name]["trace"] if isinstance(t, list)]
    plans = DC.plan_walk(case, name, DC.CASES[case]["B"])
    assert len(plans) == len(layers)
    for i, (p, entries) in enumerate(zip(plans, layers)):
        where = f"{case}/{name} layer {i}: {p} against {entries}"
        assert p.aiw == any(e in ("gn_conv_affine_pack", "gn_conv_affine_pack_wino") for e in entries), where
        assert p.wino == entries[-1].startswith("gn_conv3d_gcr_split_wino"), where
        assert p.poly == ("gn_upconv_partial" in entries), where
        assert bool(p.small) == ("gn_grid_tile_flags" in entries), where
        assert (p.mode == CONV_FP32) == (entries[-1] == "gn_conv3d_gcr"), where
    # the decision never reads the batch size: a garment's bits must not depend on how many garments share its batch
    assert DC.plan_walk(case, name, 1) == DC.plan_walk(case, name, 16) == plans


def test_the_cases_reach_every_branch():
    """what the cases were chosen for, read off the plans: both operand forms with and without Winograd, polyphase into the direct and the Winograd
    kernel, a skip connection at rest, small volumes of both edges, a dense layer behind a known rest value"""
    seen = set()
    for case in DC.CASES:
        for name in DC.ARITHS:
            seen |= {(p.aiw, p.wino, p.poly, p.small) for p in DC.plan_walk(case, name, 2) if p.mode != CONV_FP32}
    for want in ((True, True, False, 8), (True, False, False, 5), (True, True, False, 0), (True, False, False, 0), (False, True, False, 0),
                 (False, False, False, 0), (False, False, True, 0), (False, True, True, 0), (True, False, True, 0), (True, True, True, 0),
                 (False, True, False, 8), (False, False, False, 5)):
        assert want in seen, want
