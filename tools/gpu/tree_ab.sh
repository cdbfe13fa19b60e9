# Same-box bench of earlier trees (git worktrees with their own built library, e.g. ab_r05/, ab_r06b/) against this
# one, interleaved:   [SRPDE_OUT=DIR] bash tools/gpu/tree_ab.sh TAG REPS DIR...
set -o pipefail
T=$1; N=$2; shift 2
R=$(cd "$(dirname "$0")/../.." && pwd)
cd $R
O=$(realpath -m ${SRPDE_OUT:-bench_out}); mkdir -p $O
export TMPDIR=/tmp
for rep in $(seq 1 $N); do
  for v in "$@" .; do
    tag=$(basename $(cd $v && pwd))
    (cd $v && timeout -k 10 200 python bench.py $(grep -q -e --full bench.py && echo --full) --no-cpu-baseline --no-live-traffic --steps 20 --warmup 3) > $O/tab_${T}_${tag}_$rep.json 2> $O/tab_${T}_${tag}_$rep.err || { echo "bench $v failed"; tail $O/tab_${T}_${tag}_$rep.err; exit 1; }
    echo "$v $rep $(python -c "import json; d=json.load(open('$O/tab_${T}_${tag}_$rep.json')); f=d['roofline']['forward']; print(d['ms_per_step'], d['value'], f['eval']['ms'], f['train']['ms'])")"
  done
done
