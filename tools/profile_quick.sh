cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
# output directory (absolute: tools/profile_bench.py writes its part under it too)
export PV_PROFILE_OUT=$(realpath -m "${PV_PROFILE_OUT:-profile_out}")
OUT=$PV_PROFILE_OUT
mkdir -p $OUT/round $OUT/prof_one
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_one -- python3 bench.py --steps 10 --warmup 2 --full --no-cpu-baseline --no-train-forward --one-stream > $OUT/prof_one/bench.json 2> $OUT/prof_one/err.txt
find $OUT/prof_one -name "*kernel_trace.csv" -delete
find $OUT/prof_one -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/round/onestream_kernel_stats.csv
python3 bench.py --full --no-cpu-baseline > $OUT/round/bench_default.json 2> $OUT/round/bench_default.err
tail -1 $OUT/round/bench_default.json | cut -c1-600
head -30 $OUT/round/onestream_kernel_stats.csv | cut -c1-160
