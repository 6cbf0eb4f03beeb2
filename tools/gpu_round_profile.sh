# One GPU visit: GPU parity suite, FETCH_SIZE / WRITE_SIZE PMC passes ->
# pmc_traffic.json, the full bench line (with CPU baseline), rocprofv3
# kernel stats.  Results under $OUT (default bench_out/; copied to profiles/ by hand).
set -e
cd "$(dirname "$0")/.."
out=${OUT:-bench_out}
mkdir -p $out
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $out/gpu_all.log 2>&1
timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $out/pf -o pf -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $out/pf.log 2>&1
timeout -k 10 200 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $out/pw -o pw -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $out/pw.log 2>&1
python3 tools/make_traffic.py $out/pf/pf_counter_collection.csv $out/pw/pw_counter_collection.csv --config mono640 --batch 512 --algorithmic 803777536 --out $out/pmc_traffic.json > $out/traffic.log 2>&1
timeout -k 10 300 python bench.py --full --traffic-json $out/pmc_traffic.json > $out/bench_full.log 2>&1
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $out/ks -o ks -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $out/ks.log 2>&1
echo ALLDONE
