#!/usr/bin/env python3
"""Golden workspace and pack sizes (no GPU needed: the size functions are host code): workspace_bytes.json.

Run:  python tests/golden/make_golden_workspace_bytes.py --commit <sha> [--out PATH]

at the commit whose sizes are the ones to hold later refactors to -- the parent of the change that wrote every workspace layout once, as a
carve function -- and ONLY there: the file states what that code answered, so regenerating it from newer code would make
tests/test_workspace_bytes_host.py compare the code with itself.  Every gn_*_workspace_bytes / gn_*_bytes entry of the C ABI is asked over
CASES: per entry the smallest legal shape, odd and ragged shapes (so that alignment pads matter), shapes of the real workloads (32^3 and 128^3
volumes, 6000 points, B = 1 and 24) and the arguments the entry answers with 0.  gn_conv_affine_pack_workspace_bytes did not exist at that
commit: its rows hold the expression the entry and ops.conv_affine_pack both wrote out then, B * Cin * 12 + B * Cout * 4 (0 where the
sibling gn_conv_affine_pack_bytes refuses).  Only DATA is written: entry names, arguments, byte counts.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from garmentnets_amd import _lib  # noqa: E402

GOLDEN = os.path.join(HERE, "workspace_bytes.json")
MAX, MEAN, SUM, MIN, MUL = range(5)                 # GN_REDUCE_*
BF16X2, BF16X3, F16X2 = 2, 3, 4                     # GN_SPLIT_*
VOLS = [(2, 2, 2), (5, 6, 7), (32, 32, 32), (128, 128, 128)]
CONV = [(1, 1, 1, 1, 16, 32), (3, 8, 8, 8, 16, 32), (2, 5, 6, 7, 20, 32), (1, 32, 32, 32, 64, 32), (24, 32, 32, 32, 32, 64),
        (1, 128, 128, 128, 32, 32), (1, 8, 8, 8, 16, 33), (0, 8, 8, 8, 16, 32), (1, 0, 8, 8, 16, 32)]
ROWS = [(1, 1), (5, 7), (513, 3), (1025, 130), (6000, 128), (24 * 6000, 128), (0, 8), (8, 0)]
PACKS = [(1, 16, 32), (24, 16, 32), (3, 48, 96), (1, 128, 128), (24, 64, 32), (0, 16, 32), (1, 8, 32), (1, 16, 48), (-1, 16, 32)]
# a host table of gn_nocs_bin_metrics / gn_value_losses: one row count per set (the only field the size functions read)
TABLES = [[1], [5, 7], [255, 256, 257], [6000], [6000] * 8, [24 * 6000, 24 * 6000 * 3], [0], [], [1] * 9]

CASES = {
    "gn_fps_workspace_bytes": [(1, 1), (2, 4097), (1, 6000), (24, 6000), (3, 12001), (0, 6000), (1, 0)],
    "gn_grid_scatter_workspace_bytes": [(n, c, r) for r in (MAX, MEAN, SUM, MIN, MUL) for n, c in ((1, 1), (7, 4), (6000, 131), (24 * 6000, 131), (0, 4))],
    "gn_conv3d_occupancy_workspace_bytes": [(1, 1, 1, 1), (2, 8, 8, 8), (3, 5, 9, 17), (1, 32, 32, 32), (24, 32, 32, 32), (1, 128, 128, 128),
                                            (0, 8, 8, 8), (-1, 8, 8, 8), (1, 0, 8, 8)],
    "gn_conv_affine_pack_bytes": PACKS,
    "gn_conv_affine_pack_wino_bytes": PACKS,
    "gn_conv_affine_pack_workspace_bytes": PACKS,
    "gn_weight_pack_split_bytes": [(c, o, m) for m in (BF16X2, BF16X3, F16X2, 0) for c, o in ((16, 32), (48, 96), (128, 128), (64, 32), (8, 32), (16, 48))],
    "gn_weight_pack_split_wino_bytes": [(16, 32), (48, 96), (128, 128), (64, 32), (8, 32), (16, 48), (0, 32)],
    "gn_weight_pack_upconv_bytes": [(16, 32), (48, 96), (128, 64), (256, 128), (8, 32), (16, 48), (0, 32)],
    "gn_ggm3d_range_workspace_bytes": [(b,) + v for b in (1, 24) for v in VOLS + [(1, 1, 1)]] + [(0, 32, 32, 32), (-1, 32, 32, 32)],
    "gn_mc33_workspace_bytes": VOLS + [(3, 2, 9), (1, 8, 8), (8, 8, 1)],
    "gn_mc33_batch_workspace_bytes": [(b,) + v for b in (1, 2, 24) for v in VOLS] + [(3, 3, 2, 9), (0, 8, 8, 8), (1, 1, 8, 8), (2, 8, 8, 1)],
    "gn_mesh_compact_workspace_bytes": [(0, 0), (1, 1), (5, 7), (7, 5), (2049, 4100), (6000, 12000), (150000, 300000)],
    "gn_mesh_largest_component_workspace_bytes": [(0,), (1,), (5,), (6,), (6000,), (150001,), (-1,)],
    "gn_query_targets_workspace_bytes": [(b, m, f, k) for k in (0, 1, 2, 3) for b, m, f in ((1, 1, 0), (2, 5, 5), (3, 7, 2049), (1, 6000, 12000), (24, 6000, 12000))]
                                        + [(0, 5, 5, 2), (2, 0, 5, 2), (2, 5, -1, 2), (2, 5, 5, 4), (2, 5, 5, -1)],
    "gn_nocs_bin_metrics_workspace_bytes": TABLES,
    "gn_value_losses_workspace_bytes": TABLES,
    "gn_grid_scatter_bwd_workspace_bytes": [(n, c, cells, r) for r in (MAX, MEAN, SUM, MIN, MUL)
                                            for n, c, cells in ((1, 1, 1), (7, 4, 27), (6000, 131, 32 ** 3), (24 * 6000, 131, 24 * 32 ** 3), (0, 4, 27))],
    "gn_sa_gather_bwd_workspace_bytes": [(0, 1), (1, 1), (7, 5), (6000 * 64, 6000), (24 * 6000 * 64, 24 * 6000), (7, 0), (-1, 5)],
    "gn_knn_interpolate_bwd_workspace_bytes": [(0, 1, 1), (1, 1, 1), (5, 3, 7), (6000, 3, 1500), (24 * 6000, 3, 24 * 1500), (5, 0, 7), (5, 3, 0), (-1, 3, 7)],
    "gn_trilinear_sample_bwd_workspace_bytes": [(1, 0, 1, 1, 1), (1, 1, 1, 1, 1), (1, 5, 3, 4, 5), (1, 6000, 32, 32, 32), (24, 6000, 32, 32, 32),
                                                (1, 6000, 128, 128, 128), (0, 5, 3, 4, 5), (1, -1, 3, 4, 5), (1, 5, 0, 4, 5)],
    "gn_conv3d_bwd_weight_workspace_bytes": CONV,
    "gn_conv3d_bwd_weight_split_workspace_bytes": CONV,
    "gn_relu_mask_max_workspace_bytes": [(1,), (3,), (24,), (0,), (-1,)],
    "gn_groupnorm_bwd_stats_workspace_bytes": [(1, 1, 1), (3, 5 * 6 * 7, 20), (1, 32 ** 3, 64), (24, 32 ** 3, 32), (1, 128 ** 3, 32), (0, 8, 8), (1, 0, 8), (1, 8, 0)],
    "gn_linear_act_bwd_workspace_bytes": ROWS,
    "gn_linear_bwd_weight_workspace_bytes": [(m, n, k) for (m, n), k in zip(ROWS, (1, 3, 130, 5, 64, 256, 8, 8))] + [(8, 8, 0)],
    "gn_col_moments_workspace_bytes": ROWS,
    "gn_col_dots_workspace_bytes": ROWS,
    "gn_bn_train_bwd_workspace_bytes": ROWS,
    "gn_cloth_contact_workspace_bytes": [(0, 0, 0), (1, 1, 64), (12, 2, 64), (100, 3, 128), (6000, 1, 16384), (24 * 6000, 24, 16384), (12, 2, 3),
                                         (-1, 2, 64), (12, -1, 64), (12, 2, -1)],
}


def ask(lib, entry, args):
    """the entry's answer for one row of CASES"""
    if entry in ("gn_nocs_bin_metrics_workspace_bytes", "gn_value_losses_workspace_bytes"):
        cls = _lib.NocsBinSet if "nocs" in entry else _lib.LossSegment
        tab = (cls * max(len(args), 1))(*[cls(None, None, int(n), 0, 0) for n in args])
        return int(getattr(lib, entry)(tab if args else None, len(args)))
    return int(getattr(lib, entry)(*args))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit this runs at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=HERE, text=True).strip()
    lib = _lib.load()
    missing = sorted(n for n in _lib.PROTOTYPES if n.endswith("_bytes") and n not in CASES)
    if missing:
        sys.exit(f"not written: no cases for {missing}")
    rows = []
    for entry, cases in CASES.items():
        for args in cases:
            if entry == "gn_conv_affine_pack_workspace_bytes" and entry not in _lib.PROTOTYPES:
                B, cin, cout = args
                n = B * cin * 12 + B * cout * 4 if lib.gn_conv_affine_pack_bytes(B, cin, cout) else 0
            else:
                n = ask(lib, entry, args)
            rows.append([entry, list(args), n])
    with open(a.out, "w") as f:
        f.write('{"commit": ' + json.dumps(commit) + ', "rows": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
    print(f"wrote {a.out}: {len(rows)} rows of {len(CASES)} entries at {commit}")


if __name__ == "__main__":
    main()
