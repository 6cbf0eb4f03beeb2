# parity subset, full bench line, loop-burst bench (all mixes) + its rocprof summary
set -e
cd "$(dirname "$0")/.."
out=${OUT:-bench_out}
mkdir -p $out
export TMPDIR=/tmp
tag=${1:-r2d}
timeout -k 10 300 python -u -m pytest -x -q --timeout 120 --timeout-method thread -m gpu tests/test_gpu_parity.py tests/test_frame.py > $out/${tag}_par.log 2>&1
timeout -k 10 400 python -u bench.py --full > $out/${tag}_bench.log 2>&1
timeout -k 10 300 python -u bench.py --full --config loopburst > $out/${tag}_loop.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_loopks -o ks -- python3 bench.py --full --config loopburst --steps 5 --warmup 1 --no-cpu-baseline > $out/${tag}_loopks.log 2>&1
echo ALLDONE
