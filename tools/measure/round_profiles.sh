# What profiles/r01/v4_* were made with: GPU tests, default bench, bench under rocprofv3 --kernel-trace --stats, and the
# -DLNR_PROF phase profile.  Outputs under measure_out/v4/.
cd "$(dirname "$0")/../.." && export TMPDIR=/tmp && mkdir -p measure_out/v4
timeout -k 10 300 python -m pytest tests -m gpu -x -q > measure_out/v4/gpu_tests.log 2>&1 || { tail -20 measure_out/v4/gpu_tests.log; exit 1; }
tail -1 measure_out/v4/gpu_tests.log
timeout -k 10 400 python3 bench.py --full > measure_out/v4/bench_default.json 2> measure_out/v4/bench_default.log || { tail -5 measure_out/v4/bench_default.log; exit 1; }
cat measure_out/v4/bench_default.json
rm -rf measure_out/v4/prof
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d measure_out/v4/prof -- python3 bench.py --full --steps 4 --warmup 2 --no-cpu-baseline > measure_out/v4/bench_under_rocprof.json 2> measure_out/v4/bench_under_rocprof.log || exit 1
cat measure_out/v4/bench_under_rocprof.json
cp $(ls measure_out/v4/prof/*/*kernel_stats.csv | tail -1) measure_out/v4/kernel_stats.csv
head -12 measure_out/v4/kernel_stats.csv | cut -c1-160
timeout -k 10 300 python3 tools/prof_job_phases.py 100000 > measure_out/v4/phases.log 2>&1; grep -E "^==|biggest" measure_out/v4/phases.log | cut -c1-300
