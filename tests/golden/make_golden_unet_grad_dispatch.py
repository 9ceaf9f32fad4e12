#!/usr/bin/env python3
"""Golden launch trace of the UNet's training path (needs the GPU): unet_grad_dispatch_trace.json.

Run:  python tests/golden/make_golden_unet_grad_dispatch.py --commit <sha> [--out PATH]

at the commit whose training path is the one to hold later refactors to -- the parent of the change that keyed every weight pack by one generation
rule -- and ONLY there: the file states what that code launched, so regenerating it from newer code would make tests/test_gpu_unet_grad_dispatch.py
compare the code with itself.  Every case of tests/unet_grad_dispatch_cases.py runs twice under every arithmetic.  If the two runs differ in their
launches or scalar arguments, or the second run builds a pack, the file is not written.  A tensor whose bits move between the two runs has its hash
left out and is named under "unstable" (the fp64 tests hold its values).  Only DATA is written: entry and kernel names, hashes, counts.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import unet_grad_dispatch_cases as GC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit this runs at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=GC.GOLDEN)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=HERE, text=True).strip()
    traces, cases, unstable, refused = [], {}, [], []
    for case in GC.CASES:
        cases[case] = {}
        for name in GC.ARITHS:
            first, second = GC.record(case, name)[-1]
            for key in ("trace", "scalars"):
                if first[key] != second[key]:
                    refused.append(f"{case}/{name}: {key} differs between two runs")
            if second["pack_builds"] != 0:
                refused.append(f"{case}/{name}: the second run built {second['pack_builds']} packs")
            rec = dict(scalars=second["scalars"], pack_scalars=first["pack_scalars"], pack_builds=[first["pack_builds"], second["pack_builds"]])
            if first["out"] == second["out"]:
                rec["out"] = second["out"]
            else:
                unstable.append(f"{case}/{name}: out")
            rec["grads"] = {}
            for n, h in second["grads"].items():
                if first["grads"][n] == h:
                    rec["grads"][n] = h
                else:
                    unstable.append(f"{case}/{name}: grad {n}")
            if second["trace"] not in traces:
                traces.append(second["trace"])
            cases[case][name] = dict(rec, trace=traces.index(second["trace"]))
            print(f"{case}/{name}: {len(second['trace'])} calls, {first['pack_builds']} pack builds in the first run, {second['pack_builds']} in the "
                  f"second, {len(rec['grads'])} gradient hashes", flush=True)
    if refused:
        sys.exit("not written:\n  " + "\n  ".join(refused))
    with open(args.out, "w") as f:
        json.dump(dict(commit=commit, unstable=unstable, traces=traces, cases=cases), f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes) at {commit}; unstable: {unstable or 'none'}")


if __name__ == "__main__":
    main()
