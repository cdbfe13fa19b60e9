# Poisson tests (spsolve fixtures, cooperative vs polled grid CG, cascade / report users) and the
# config #3 bench line:  [SRPDE_OUT=DIR] bash tools/gpu/poisson_final.sh TAG
set -o pipefail
T=${1:-p}
R=$(cd "$(dirname "$0")/../.." && pwd)
cd $R
O=$(realpath -m ${SRPDE_OUT:-bench_out}); mkdir -p $O
timeout -k 10 300 python -u -m pytest tests/test_gpu_poisson.py tests/test_gpu_cascade.py tests/test_gpu_poisson_rows.py tests/test_gpu_report.py -x -q --timeout 120 --timeout-method thread -m gpu > $O/poisson_$T.log 2>&1 || { echo "tests failed"; tail -30 $O/poisson_$T.log; exit 1; }
tail -1 $O/poisson_$T.log
timeout -k 10 300 python bench.py --full --workload poisson > $O/bench_poisson_$T.json 2> $O/bench_poisson_$T.err || { echo "bench failed"; tail $O/bench_poisson_$T.err; exit 1; }
cat $O/bench_poisson_$T.json
timeout -k 10 300 python bench.py --full --workload poisson --no-cpu-baseline --poisson-sizes 640:1 > $O/bench_poisson640b1_$T.json 2>> $O/bench_poisson_$T.err || { echo "bench 640 failed"; exit 1; }
cat $O/bench_poisson640b1_$T.json
