"""GPU (-m gpu): the UNet's conv dispatch launches what it launched before conv_plan existed.

tests/golden/unet_dispatch_trace.json was recorded at the parent of the change that introduced conv_plan (golden/make_golden_unet_dispatch.py): per case
and arithmetic of tests/unet_dispatch_cases.py the library entries and kernels per layer, a hash of every call's scalar arguments, the hashes of the
pre-final volume and its statistics, and the number of weight packs built by a second run of the same model.  The same cases run through the present
code must reproduce all four: a refactor of the host code issues the same launches and gives the same bits."""
import pytest

pytestmark = pytest.mark.gpu

import unet_dispatch_cases as DC  # noqa: E402

GOLDEN = DC.load_golden()


@pytest.mark.parametrize("case", list(DC.CASES))
def test_unet_dispatch_reproduces_the_recorded_launches(case):
    for name in DC.ARITHS:
        want = GOLDEN["cases"][case][name]
        first, second = DC.record(case, name)
        for got in (first, second):
            assert got["trace"] == want["trace"], f"{case}/{name}: launches differ"
            assert got["scalars"] == want["scalars"], f"{case}/{name}: scalar arguments differ"
            assert got["out"] == want["out"] and got["stats"] == want["stats"], f"{case}/{name}: same launches, other bits"
        assert second["pack_builds"] == want["pack_builds"] == 0, f"{case}/{name}: a pack was rebuilt on a second call"
