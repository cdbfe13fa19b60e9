# Whole GPU suite + smoke + the full bench line (roofline, CPU baseline) on one MI355X box.
#   [SRPDE_OUT=DIR] bash tools/gpu/full.sh TAG     (logs under DIR, default bench_out/ in the repository)
set -o pipefail
T=${1:-full}
R=$(cd "$(dirname "$0")/../.." && pwd)
cd $R
O=$(realpath -m ${SRPDE_OUT:-bench_out}); mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -x -q --timeout 180 --timeout-method thread -m gpu > $O/pytest_$T.log 2>&1 || { echo "pytest failed"; grep -v amdgpu $O/pytest_$T.log | tail -30; exit 1; }
tail -1 $O/pytest_$T.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$T.log 2>&1 || { echo "smoke failed"; tail -20 $O/smoke_$T.log; exit 1; }
tail -1 $O/smoke_$T.log
timeout -k 10 400 python bench.py --full > $O/bench_$T.json 2> $O/bench_$T.err || { echo "bench failed"; tail -20 $O/bench_$T.err; exit 1; }
cat $O/bench_$T.json
