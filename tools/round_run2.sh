# round-end evidence beyond the driver's command: boundary-A kernel profile, configs 3 / 4 / 5, the 363-complex stream (config 4)
OUT=${1:?usage: tools/round_run2.sh <output directory>}
mkdir -p "$OUT"
bash tools/profile_tp.sh > "$OUT"/profile_tp.log 2>&1; tail -5 "$OUT"/profile_tp.log
for c in 3 4 5; do
  python bench.py --full --config $c --steps 20 --warmup 5 --no-cpu-baseline --no-alt --no-device-loop --no-timesplit > "$OUT"/bench_config${c}_n1.json 2> "$OUT"/bench_config${c}.err
  python tools/show_bench.py "$OUT"/bench_config${c}_n1.json | head -4
done
python bench.py --full --config 4 --complexes 363 --steps 363 --warmup 2 --no-cpu-baseline --no-alt --no-device-loop --no-timesplit > "$OUT"/bench_config4_363.json 2> "$OUT"/bench_config4_363.err
python tools/show_bench.py "$OUT"/bench_config4_363.json | head -4
