OUT=${1:?usage: tools/round_run1.sh <output directory>}
mkdir -p "$OUT"
( time python bench.py --full --steps 20 --warmup 5 > "$OUT"/bench_n1.json 2> "$OUT"/bench_n1.err ) 2> "$OUT"/bench_n1.time
tail -c 600 "$OUT"/bench_n1.err; cat "$OUT"/bench_n1.time
bash tools/profile_round.sh > "$OUT"/profile_round.log 2>&1
ls gpurun_out/prof_summary
