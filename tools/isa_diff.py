#!/usr/bin/env python3
"""Compare the gfx950 device code of two csrc directories, kernel by kernel.

    tools/isa_diff.py OLD_CSRC NEW_CSRC [--jobs N] [--keep DIR]

Every .hip file of both directories is compiled to device assembly with the Makefile's flags (the directories must sit two levels below
an include/ folder, as garmentnets_amd/csrc does).  A kernel is the text between its `_Z...:` label and the next one; comment lines and
.file/.ident/.loc lines are ignored, and so is the function number in local labels (.LBB12_3: adding or removing a kernel renumbers those below it).  Prints one line per kernel that differs (instruction counts and the five resource values of its
metadata, old -> new) and a summary; the exit status is 1 when any kernel differs, was added or was removed.  For a kernel with matrix
instructions the line also says whether the two streams are equal up to and including the kernel's last v_mfma: "main loop equal" means that
only the epilogue behind it was re-scheduled, "main loop DIFFERS" that the change reached the loop itself.
"""
import argparse, concurrent.futures as cf, os, re, subprocess, sys, tempfile

FLAGS = "-O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -Wall -Wno-unused-function --cuda-device-only -S".split()
UNROLL = {"decode_split.hip", "unet_wino.hip", "unet_wino32.hip"}  # the Makefile's per-file addition
RES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def compile_asm(src, out):
    extra = ["-mllvm", "-pragma-unroll-threshold=200000"] if os.path.basename(src) in UNROLL else []
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *FLAGS, *extra, src, "-o", out], check=True, cwd=os.path.dirname(src))
    return out


def kernels(path):
    """{symbol: (code lines, resource dict)} of one assembly file; device functions and variables that were not inlined count as symbols too"""
    text = open(path).read()
    body, cur = {}, None
    for line in text.split("\n"):
        s = line.split(";")[0].strip()
        m = re.match(r"(_Z\w+):", s)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif s.startswith(".type") or s.startswith(".section"):  # the next symbol, or the end of the text
            cur = None
        elif cur and s and not re.match(r"\.(file|ident|loc)\b", s):
            body[cur].append(re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", s))  # local labels carry the function's number within its file
    res = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = {k: re.search(re.escape(k) + r":\s+(\S+)", blk).group(1) for k in RES}
    return {k: (v, res.get(k, {})) for k, v in body.items()}


def through_last_mfma(code):
    """the code lines up to and including the last matrix instruction (None: the kernel has none)"""
    last = max((i for i, l in enumerate(code) if l.startswith("v_mfma")), default=None)
    return None if last is None else code[:last + 1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old"), ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", help="write the assembly files here (old/ and new/) instead of a temporary folder")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    jobs = []
    with cf.ThreadPoolExecutor(a.jobs) as ex:
        for tag, d in (("old", a.old), ("new", a.new)):
            os.makedirs(os.path.join(tmp, tag), exist_ok=True)
            for f in sorted(os.listdir(d)):
                if f.endswith(".hip"):
                    jobs.append((tag, f, ex.submit(compile_asm, os.path.abspath(os.path.join(d, f)), os.path.join(tmp, tag, f[:-4] + ".s"))))
    asm = {"old": {}, "new": {}}
    for tag, f, j in jobs:
        asm[tag][f] = kernels(j.result())
    same = bad = 0
    for f in sorted(set(asm["old"]) | set(asm["new"])):
        o, n = asm["old"].get(f, {}), asm["new"].get(f, {})
        for k in sorted(set(o) | set(n)):
            if k not in o or k not in n:
                print(f"{f}: {k}: {'ADDED' if k in n else 'REMOVED'}")
                bad += 1
            elif o[k][0] == n[k][0] and o[k][1] == n[k][1]:
                same += 1
            else:
                res = " ".join(f"{r[1:]}={o[k][1].get(r)}->{n[k][1].get(r)}" for r in RES)
                cnt = [sum(1 for l in x[k][0] if l[0] != "." and l[-1] != ":") for x in (o, n)]
                head = [through_last_mfma(x[k][0]) for x in (o, n)]
                loop = "" if head[0] is None and head[1] is None else (" main loop equal" if head[0] == head[1] else " main loop DIFFERS")
                print(f"{f}: {k}: DIFFERS instructions {cnt[0]}->{cnt[1]} {res}{loop}")
                bad += 1
    print(f"{same} kernels identical, {bad} differ / added / removed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
