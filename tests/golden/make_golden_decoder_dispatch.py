#!/usr/bin/env python3
"""Golden launch trace of the implicit decoder's dispatch (needs the GPU): decoder_dispatch_trace.json.

Run:  python tests/golden/make_golden_decoder_dispatch.py --commit <sha> [--out PATH]

at the commit whose dispatch is the one to hold later refactors to -- the parent of the change that introduced decode_plan -- and ONLY there: the file
states what that code launched, so regenerating it from newer code would make tests/test_gpu_decoder_dispatch.py compare the code with itself.
Every case of tests/decoder_dispatch_cases.py (source x decoder x call) runs twice under every arithmetic; if the two runs differ in anything the file
is not written.  Only DATA is written: entry names, hashes, counts.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import decoder_dispatch_cases as DC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit this runs at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=DC.GOLDEN)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=HERE, text=True).strip()
    traces, cases, unstable = [], {}, []
    for src in DC.SOURCES:
        for dec in ("256x1", "256x3"):
            flags = DC.unsafe_flags(src, dec)
            if flags != [0.0, 1.0]:
                sys.exit(f"not written: {src}/{dec}: the device's unsafe flags are {flags}, the cases want garment 1 alone on the gated fp32 twin")
        for dec in DC.DECODERS:
            for call in DC.CALLS:
                case = cases[DC.case_id(src, dec, call)] = {}
                for name in DC.ARITHS:
                    first, second = DC.record(src, dec, call, name)
                    for key in ("trace", "scalars", "out"):
                        if first[key] != second[key]:
                            unstable.append(f"{DC.case_id(src, dec, call)}/{name}: {key} differs between two runs")
                    if second["trace"] not in traces:
                        traces.append(second["trace"])
                    case[name] = dict(second, trace=traces.index(second["trace"]))
                    print(f"{DC.case_id(src, dec, call)}/{name}: {[len(c) for c in DC.calls_of(second['trace'])]} entries per call, "
                          f"{second['pack_builds']} pack builds in the second run ({first['pack_builds']} in the first)", flush=True)
    if unstable:
        sys.exit("not written:\n  " + "\n  ".join(unstable))
    with open(args.out, "w") as f:
        json.dump(dict(commit=commit, traces=traces, cases=cases), f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes) at {commit}")


if __name__ == "__main__":
    main()
