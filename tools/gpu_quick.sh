set -u
OUT="${OUT:-out}"  # where the logs and result lines go
mkdir -p "$OUT"
TSG_STAMPS=1 TSG_TRACE=1 timeout -k 10 600 python bench.py --full --steps 5 --warmup 2 --cpu-baseline 0 > $OUT/stamps.json 2> $OUT/stamps.err || exit $?
grep "stamps" $OUT/stamps.err | tail -4
TSG_TRACE=1 timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 --cpu-baseline 0 > $OUT/trace.json 2> $OUT/trace.err || exit $?
grep "\[tsg\]" $OUT/trace.err | tail -4
timeout -k 10 600 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err || exit $?
cat $OUT/bench.json
