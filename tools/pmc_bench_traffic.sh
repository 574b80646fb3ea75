#!/bin/bash
# HBM traffic of the bench's dominant kernel, per launch: FETCH_SIZE and WRITE_SIZE in SEPARATE rocprofv3 --pmc
# passes (kernel-trace only: both do not fit one pass), over the bench's own command line in engine-only mode, then
# summarised into profiles/r3_traffic.json (read by bench.py --full for roofline.traffic).
# Usage (on a machine with the GPU):  [OUT=<folder>] bash tools/pmc_bench_traffic.sh [c3|c2] [h2|bx3|tap]
WL=${1:-c3}
IMPL=${2:-h2}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/build/pmc_traffic}
mkdir -p "$OUT"
export TMPDIR=${TMPDIR:-$OUT}
cd "$OUT"
# the per-op profile belongs to the roofline leg of a --full run; the counter passes need the engine-only steps alone
timeout 900 python $R/bench.py --full --workload $WL --impl $IMPL --steps 1 --warmup 1 --no-cpu-baseline --engine-only --no-compare --traffic static --dump-ops "$OUT/ops_$WL.csv" > "$OUT/bench_ops_$WL.json" 2> "$OUT/bench_ops_$WL.err"
for C in FETCH_SIZE WRITE_SIZE; do
  rm -rf "$OUT/pmc_bench_$C"
  timeout 600 rocprofv3 --kernel-trace --pmc $C --output-format csv -d "$OUT/pmc_bench_$C" -o p -- \
      python $R/bench.py --workload $WL --impl $IMPL --steps 1 --warmup 1 --engine-only > "$OUT/pmc_bench_$C.log" 2>&1
  echo "pass $C rc=$?"
done
cd $R
python tools/pmc_traffic_summary.py $WL "$OUT/ops_$WL.csv" "$OUT/pmc_bench_FETCH_SIZE" "$OUT/pmc_bench_WRITE_SIZE" $IMPL
