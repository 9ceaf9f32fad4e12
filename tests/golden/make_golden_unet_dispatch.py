#!/usr/bin/env python3
"""Golden launch trace of the UNet's conv dispatch (needs the GPU): unet_dispatch_trace.json.

Run:  python tests/golden/make_golden_unet_dispatch.py --commit <sha> [--out PATH]

at the commit whose dispatch is the one to hold later refactors to -- the parent of the change that introduced conv_plan -- and ONLY there: the file
states what that code launched, so regenerating it from newer code would make tests/test_gpu_unet_dispatch.py compare the code with itself.
Every case of tests/unet_dispatch_cases.py runs twice under every arithmetic; if the two runs differ in anything the file is not written
(the path is deterministic: tests/test_gpu_parity.py::test_run_twice_is_bit_identical).  Only DATA is written: entry and kernel names, hashes, counts.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import unet_dispatch_cases as DC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit this runs at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=DC.GOLDEN)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=HERE, text=True).strip()
    traces, cases, unstable = [], {}, []
    for case in DC.CASES:
        cases[case] = {}
        for name in DC.ARITHS:
            first, second = DC.record(case, name)
            for key in ("trace", "scalars", "out", "stats"):
                if first[key] != second[key]:
                    unstable.append(f"{case}/{name}: {key} differs between two runs")
            if second["trace"] not in traces:
                traces.append(second["trace"])
            cases[case][name] = dict(second, trace=traces.index(second["trace"]))
            print(f"{case}/{name}: {sum(isinstance(t, list) for t in second['trace'])} layers, {second['pack_builds']} pack builds in the second run "
                  f"({first['pack_builds']} in the first)", flush=True)
    if unstable:
        sys.exit("not written:\n  " + "\n  ".join(unstable))
    with open(args.out, "w") as f:
        json.dump(dict(commit=commit, traces=traces, cases=cases), f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes) at {commit}")


if __name__ == "__main__":
    main()
