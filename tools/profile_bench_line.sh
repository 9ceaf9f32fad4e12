#!/bin/bash
# The round's default bench line (bench.py --full) with a 10 Hz power / clock trace beside it, then the rocprofv3 passes (tools/profile_round.sh) and the
# secondary workloads of DESIGN.md section 5, on the GPU box.  The bench lines and logs land in <out dir> (default profile_<tag>/), the rocprofv3 summaries
# where tools/profile_round.sh puts them; copy what is to be judged into profiles/.
# usage: tools/profile_bench_line.sh <tag> [out dir]
TAG=${1:-r03}
OUT=${2:-profile_$TAG}
mkdir -p "$OUT"
python tools/power_trace.py "$OUT/${TAG}_power_bench.csv" python bench.py --full --steps 20 --warmup 5 > "$OUT/${TAG}_bench_default.json" 2> "$OUT/${TAG}_bench_default.err"
tail -c 300 "$OUT/${TAG}_bench_default.err"
bash tools/profile_round.sh ${TAG} > "$OUT/${TAG}_profile.log" 2>&1
python bench.py --full --steps 10 --warmup 3 --volume-size 256 --batch 8 --no-strict-pass --no-cpu-baseline --no-pmc --no-latency-b1 > "$OUT/${TAG}_bench_q256.json" 2> "$OUT/${TAG}_bench_q256.err"
python bench.py --full --steps 10 --warmup 3 --input noisy_wnf --no-strict-pass --no-cpu-baseline --no-pmc --no-latency-b1 > "$OUT/${TAG}_bench_noisy_wnf.json" 2> "$OUT/${TAG}_bench_noisy_wnf.err"
python bench.py --full --steps 10 --warmup 3 --workload pointnet2 --no-pmc > "$OUT/${TAG}_bench_pointnet2.json" 2> "$OUT/${TAG}_bench_pointnet2.err"
python bench.py --full --steps 10 --warmup 3 --input collapsed --no-strict-pass --no-cpu-baseline --no-pmc --no-latency-b1 > "$OUT/${TAG}_bench_collapsed.json" 2> "$OUT/${TAG}_bench_collapsed.err"
python bench.py --full --steps 10 --warmup 3 --grid 32 --reduce max --no-strict-pass --no-cpu-baseline --no-pmc --no-latency-b1 > "$OUT/${TAG}_bench_g32.json" 2> "$OUT/${TAG}_bench_g32.err"
ls gpurun_out/prof_${TAG}
