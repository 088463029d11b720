# round-end evidence on the final library (default conv kernel = two limbs / three products): the driver's command, configs 3 / 4 / 5, the 363-complex stream (config 4),
# its per-kernel profile, the 8-rank single-GPU comparison
OUT=${1:?usage: tools/round_run3.sh <output directory>}
mkdir -p "$OUT"
( time python bench.py --full --steps 20 --warmup 5 > "$OUT"/bench_n1.json 2> "$OUT"/bench_n1.err ) 2> "$OUT"/bench_n1.time
python tools/show_bench.py "$OUT"/bench_n1.json; cat "$OUT"/bench_n1.time | tail -3
for c in 3 4 5; do
  python bench.py --full --config $c --steps 20 --warmup 5 --no-cpu-baseline --no-device-loop --no-timesplit > "$OUT"/bench_config${c}_n1.json 2> "$OUT"/bench_config${c}.err
  python tools/show_bench.py "$OUT"/bench_config${c}_n1.json | head -6
done
python bench.py --full --config 4 --complexes 363 --steps 363 --warmup 2 --no-cpu-baseline --no-device-loop --no-timesplit > "$OUT"/bench_config4_363.json 2> "$OUT"/bench_config4_363.err
python tools/show_bench.py "$OUT"/bench_config4_363.json | head -6
bash tools/profile_config4.sh 48 > "$OUT"/profile_config4.log 2>&1; tail -8 "$OUT"/profile_config4.log
bash tools/ranks8_check.sh "$OUT"/ranks8.json > "$OUT"/ranks8.log 2>&1; tail -5 "$OUT"/ranks8.log
