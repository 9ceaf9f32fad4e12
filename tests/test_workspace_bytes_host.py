"""Every size entry of the C ABI answers what tests/golden/workspace_bytes.json recorded at the commit before the workspace layouts became carve
functions (tests/golden/make_golden_workspace_bytes.py says how and where it was written).  Host code only: no GPU."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_workspace_bytes as G  # noqa: E402
from garmentnets_amd import _lib  # noqa: E402

with open(G.GOLDEN) as _f:
    ROWS = json.load(_f)["rows"]


def test_every_size_entry_is_recorded():
    entries = {n for n in _lib.PROTOTYPES if n.endswith("_bytes")}
    assert entries == {e for e, _, _ in ROWS} == set(G.CASES)
    assert len(ROWS) == sum(len(c) for c in G.CASES.values())


@pytest.mark.parametrize("entry", sorted(G.CASES))
def test_sizes_are_the_recorded_ones(entry):
    lib = _lib.load()
    rows = [(a, n) for e, a, n in ROWS if e == entry]
    assert [list(a) for a in G.CASES[entry]] == [a for a, _ in rows]
    assert [(a, G.ask(lib, entry, a)) for a, _ in rows] == rows


def test_conv_affine_pack_workspace_is_the_old_expression():
    lib = _lib.load()
    for B, cin, cout in ((1, 16, 32), (24, 64, 32), (3, 48, 96)):
        assert lib.gn_conv_affine_pack_workspace_bytes(B, cin, cout) == B * cin * 12 + B * cout * 4
