#!/bin/bash
# rocprofv3 kernel-trace stats + PMC traffic passes of the bench, into $OUT/.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT="${OUT:-out}"  # where the logs and result lines go
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- \
  python3 bench.py --full --steps 20 --warmup 3 --cpu-baseline 0 ${BENCH_ARGS:-} > $OUT/prof_bench.json 2> $OUT/prof_bench.err || exit $?
echo "rocprof ok"; find $OUT/prof -name "*kernel_stats.csv" | head -1 | xargs cat
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 -s KILL 600 rocprofv3 --pmc $c -d $OUT/pmc_$c -o run --output-format csv -- \
    python3 bench.py --full --steps 10 --warmup 2 --cpu-baseline 0 ${BENCH_ARGS:-} > $OUT/pmc_$c.json 2> $OUT/pmc_$c.err || exit $?
  echo "pmc $c ok"
done
python3 tools/pmc_summary.py $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE --out $OUT/pmc_traffic.json \
  --workload "${PMC_WORKLOAD:-blocks=10,entries=1000000}" --source "${PMC_SOURCE:-tools/gpu_prof.sh}" | tee $OUT/pmc_summary.txt
