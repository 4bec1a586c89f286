#!/bin/bash
# Regenerates the evidence of a round in one GPU call (the logs of this script land in OUT, default evidence/; copy what should be judged into profiles/):
#   gpurun --timeout 3000 -- 'tools/round_end.sh r03'
# profile (kernel trace + PMC traffic + MFMA busy), the headline bench line with roofline / cpu_baseline, the other bench workloads, the GPU tests.
TAG=${1:-rnd}
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
OUT=${OUT:-evidence}      # (tools/profile.sh, tools/pmc_mfma.sh and the GPU tests' parity record keep their own output folder)
mkdir -p $OUT
tools/profile.sh $TAG > $OUT/${TAG}_profile_sh.log 2>&1
tools/pmc_mfma.sh $TAG > /dev/null 2>&1
timeout 900 python bench.py --full > $OUT/${TAG}_bench.log 2>&1
timeout 300 python bench.py --full --workload scene --steps 1 --warmup 1 --no-cpu-baseline > $OUT/${TAG}_bench_scene.log 2>&1
timeout 300 python bench.py --full --workload scene --fp8 --steps 1 --warmup 1 --no-cpu-baseline > $OUT/${TAG}_bench_scene_fp8.log 2>&1
timeout 300 python bench.py --inputs 4 --edm-steps 50 --steps 1 --warmup 0 --no-cpu-baseline --no-roofline > $OUT/${TAG}_bench_inputs4_steps50.log 2>&1
timeout 300 python bench.py --graph --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > $OUT/${TAG}_bench_graph.log 2>&1
timeout 400 python bench.py --shard-sim 8 > $OUT/${TAG}_shard_sim8.log 2>&1
timeout 400 python bench.py --shard-sim 2 > $OUT/${TAG}_shard_sim2.log 2>&1
timeout 200 python tools/op_times.py > $OUT/${TAG}_op_times.log 2>&1
timeout 200 python tools/conv_gn_bench.py > $OUT/${TAG}_conv_gn_bench.log 2>&1
timeout 400 python bench.py --shard-sim 8 --inputs 4 --edm-steps 50 > $OUT/${TAG}_shard_sim8_inputs4_steps50.log 2>&1
timeout 200 python tools/lib_gemm_probe.py > $OUT/${TAG}_lib_gemm_probe.log 2>&1
timeout 600 python tools/e4_stress.py 2000 > $OUT/${TAG}_e4_stress.log 2>&1
T0=$(date +%s)
timeout 1200 python -m pytest tests -m gpu -q --durations=12 > $OUT/${TAG}_pytest_gpu.log 2>&1      # (1200 s: the limit the suite is held to)
RC=$?
T1=$(date +%s)
cp gpurun_out/parity.json gpurun_out/${TAG}_parity.json      # (later calls start from an empty gpurun_out/ on the box: keep the full-suite record under its own name)
tail -25 $OUT/${TAG}_pytest_gpu.log
for f in bench bench_scene bench_scene_fp8 bench_inputs4_steps50 bench_graph shard_sim8 shard_sim2 shard_sim8_inputs4_steps50; do echo "== $f"; tail -c 400 $OUT/${TAG}_$f.log | head -c 400; echo; done
# the suite must fit the driver's 1200 s limit with margin (GPUTEST_r04: killed at 1200 s after 144 of 168 tests): fail the round-end run above 900 s
echo "pytest -m gpu: rc=$RC wall=$((T1 - T0)) s (limit 900)" | tee $OUT/${TAG}_pytest_gpu_wall.txt
if [ $RC -ne 0 ] || [ $((T1 - T0)) -gt 900 ]; then echo "ROUND-END FAILURE: GPU suite red or over 900 s"; exit 1; fi
