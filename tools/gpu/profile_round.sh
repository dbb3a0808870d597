#!/bin/bash
# Round profile: kernel trace + stats, PMC FETCH/WRITE passes -> traffic.json,
# PMC SQ pass, then the full bench line (which picks up traffic.json).
# The bench runs use --full: traffic.json is the finest-level search launch of
# the roofline pass (whole batch on one stream), which a plain run does not make.
# Everything is written under $OUT (default: out/ in the repository).
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/out}
cd "$R"; mkdir -p "$OUT"
TAG=${TAG:-r03}
BENCH="$R/bench.py --full --steps 10 --warmup 5 --warmup-floor 0 --no-cpu-baseline --no-tolerance-mode --no-pipelined"
cd /tmp && export TMPDIR=/tmp
run() { local name=$1; shift; timeout -k 10 400 "$@" > $OUT/$name.log 2>&1; local rc=$?; echo "$name rc=$rc"; [ $rc -eq 0 ] || { tail -5 $OUT/$name.log; exit $rc; }; }
run trace rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_trace -o run -- python3 $BENCH
run fetch rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_fetch -o run -- python3 $BENCH
run write rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/${TAG}_write -o run -- python3 $BENCH
run sq rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_ANY SQ_WAIT_ANY GRBM_GUI_ACTIVE --output-format csv -d $OUT/${TAG}_sq -o run -- python3 $BENCH
run marker rocprofv3 --marker-trace --kernel-trace --output-format csv -d $OUT/${TAG}_marker -o run -- python3 $R/bench.py --steps 3 --warmup 2 --warmup-floor 0
cd $R
python3 tools/pmc_traffic.py $OUT/${TAG}_fetch/run_counter_collection.csv $OUT/${TAG}_write/run_counter_collection.csv --out $OUT/traffic.json
python3 tools/trace_stats.py $OUT/${TAG}_trace/run_kernel_trace.csv $OUT/${TAG}_trace/kernel_grid_stats.csv
timeout -k 10 400 python3 bench.py --full --traffic-json $OUT/traffic.json > $OUT/bench_final.log 2>&1; echo "bench rc=$?"; tail -1 $OUT/bench_final.log
