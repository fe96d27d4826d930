#!/bin/bash
# end-of-round evidence on ONE box: GPU suite, rocprofv3 kernel stats (two-branch and one-stream), PMC traffic (written where bench.py reads it, so the
# default bench line that follows carries a fresh `roofline.traffic`), the default bench line, the driver-flag bench line, kbench, conv stamps
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
# output directory (absolute: tools/profile_bench.py writes its part under it too)
export PV_PROFILE_OUT=$(realpath -m "${PV_PROFILE_OUT:-profile_out}")
OUT=$PV_PROFILE_OUT
R=${PV_ROUND:-r06}
mkdir -p $OUT/round
python -m pytest tests -q -m gpu --durations=25 > $OUT/round/final_tests.txt 2>&1
tail -5 $OUT/round/final_tests.txt
python3 tools/profile_bench.py 10 > $OUT/prof_bench_stdout.txt 2>&1
cp $OUT/prof_bench/pmc_traffic.json profiles/${R}_pmc_traffic.json
cp $OUT/prof_bench/pmc_traffic.json $OUT/round/pmc_traffic.json
cp $OUT/prof_bench/kernel_stats.csv $OUT/round/default_kernel_stats.csv
cp $OUT/prof_bench/bench_under_rocprof.json $OUT/round/default_under_rocprof.json
mkdir -p $OUT/prof_one
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_one -- python3 bench.py --steps 10 --warmup 2 --full --no-cpu-baseline --no-train-forward --one-stream > $OUT/prof_one/bench.json 2> $OUT/prof_one/err.txt
find $OUT/prof_one -name "*kernel_trace.csv" -delete
find $OUT/prof_one -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/round/onestream_kernel_stats.csv
tail -1 $OUT/prof_one/bench.json > $OUT/round/onestream_under_rocprof.json
python3 bench.py --full > $OUT/round/bench_default.json 2> $OUT/round/bench_default.err
python3 bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/round/bench_driver_flags.json 2> /dev/null
tail -3 $OUT/prof_bench_stdout.txt; tail -1 $OUT/round/bench_default.json | cut -c1-400
python3 tools/kbench.py > $OUT/round/kbench.txt 2>&1
python3 tools/diag/convbig_seg_stamps.py 2>&1 | grep -v "^   [12] " > $OUT/round/convbig_stamps.txt
for part in head tail merged; do python3 tools/diag/plan_breakdown.py $part 2>&1 | grep -v amdgpu.ids > $OUT/round/plan_breakdown_$part.txt; done
PMC_PASSES=0,1,3,4,5 python3 tools/pmc.py "attn2 branch C320 n4096 FUSED" xattn_fused > $OUT/round/pmc_xfused320.txt 2>&1
PMC_PASSES=0,1,3,4,5 python3 tools/pmc.py "attn d40 n4096" attn8_kernel > $OUT/round/pmc_attn8.txt 2>&1
PMC_PASSES=0,1,3,4,5 python3 tools/pmc.py "conv3 320->320 @64" big_tile > $OUT/round/pmc_conv_patch.txt 2>&1
