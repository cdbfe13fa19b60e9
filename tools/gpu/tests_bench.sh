# The full GPU suite, smoke(), then the bench line (no CPU baseline / live traffic): a quick whole-tree check.
#   [SRPDE_OUT=DIR] bash tools/gpu/tests_bench.sh TAG
set -o pipefail
T=${1:-tb}
R=$(cd "$(dirname "$0")/../.." && pwd)
cd $R
O=$(realpath -m ${SRPDE_OUT:-bench_out}); mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -x -q --timeout 200 --timeout-method thread -m gpu > $O/tb_pytest_$T.log 2>&1 || { echo "pytest failed"; grep -v amdgpu $O/tb_pytest_$T.log | tail -40; exit 1; }
tail -1 $O/tb_pytest_$T.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/tb_smoke_$T.log 2>&1 || { echo "smoke failed"; tail -20 $O/tb_smoke_$T.log; exit 1; }
tail -1 $O/tb_smoke_$T.log
timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-live-traffic > $O/tb_bench_$T.json 2> $O/tb_bench_$T.err || { echo "bench failed"; tail -20 $O/tb_bench_$T.err; exit 1; }
python -c "import json; d=json.load(open('$O/tb_bench_$T.json')); print(d['ms_per_step'], d['value'], d['roofline']['forward']['eval']['ms'], d['roofline']['forward']['train']['ms'])"
