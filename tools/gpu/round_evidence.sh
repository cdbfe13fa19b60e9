# Round-end evidence on one MI355X: full GPU tests, smoke, HBM-traffic PMC passes for the
# roofline kernel (bridge.3 forward conv) kept as profiles/traffic_*.json, the bench line exactly as
# the driver runs it (which measures the same traffic live), and the kernel-trace stats of the bench
# command.
# usage: [SRPDE_OUT=DIR] bash tools/gpu/round_evidence.sh TAG     (outputs under DIR, default bench_out/; copy what is judged to profiles/)
set -o pipefail
T=${1:-final}
R=$(cd "$(dirname "$0")/../.." && pwd)
cd $R
O=$(realpath -m ${SRPDE_OUT:-bench_out}); mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -x -q --timeout 120 --timeout-method thread -m gpu > $O/pytest_$T.log 2>&1 || { echo "pytest failed"; grep -v amdgpu $O/pytest_$T.log | tail -30; exit 1; }
tail -1 $O/pytest_$T.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$T.log 2>&1 || { echo "smoke failed"; tail -20 $O/smoke_$T.log; exit 1; }
tail -1 $O/smoke_$T.log
cd /tmp
i=0
for C in FETCH_SIZE WRITE_SIZE; do
  i=$((i+1))
  timeout -k 10 120 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $O/pmc_$T -o p$i -- python $R/tools/conv_bench.py --layers bridge.3 --only fwd --iters 3 > $O/pmc_${T}_$i.log 2>&1 || { echo "pmc pass $i failed"; exit 1; }
done
cd $R
O=$(realpath -m ${SRPDE_OUT:-bench_out}); mkdir -p $O
python tools/traffic_json.py $O/pmc_$T bridge.3 $O/traffic_$T.json
timeout -k 10 500 python bench.py --full > $O/bench_$T.json 2> $O/bench_$T.err || { echo "bench failed"; tail -20 $O/bench_$T.err; exit 1; }
cat $O/bench_$T.json
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$T -o bench -- python $R/bench.py --no-cpu-baseline --no-live-traffic > $O/prof_$T.log 2>&1 || { echo "prof failed"; exit 1; }
echo "round evidence done"
