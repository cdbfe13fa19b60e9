set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd)
cd $R
O=$(realpath -m ${SRPDE_OUT:-bench_out}); mkdir -p $O
timeout -k 10 500 python -u -m pytest tests/test_gpu_kernels.py tests/test_gpu_unet.py tests/test_gpu_b1024.py tests/test_gpu_schedule.py tests/test_gpu_train.py -x -q --timeout 120 --timeout-method thread -m gpu > $O/oc2_pytest.log 2>&1 || { echo "tests failed"; grep -v amdgpu $O/oc2_pytest.log | tail -40; exit 1; }
tail -1 $O/oc2_pytest.log
timeout -k 10 120 python tools/conv_bench.py --layers out_conv1,out_conv2,enc1.conv2 --iters 20 > $O/oc2_conv.log 2>&1 || { echo "conv_bench failed"; tail -20 $O/oc2_conv.log; exit 1; }
cat $O/oc2_conv.log
for r in 1 2 3; do
timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-live-traffic --steps 20 > $O/oc2_bench_$r.json 2> $O/oc2_bench_$r.err || { echo "bench failed"; tail $O/oc2_bench_$r.err; exit 1; }
python -c "import json; d=json.load(open('$O/oc2_bench_$r.json')); print(d['ms_per_step'], d['value'], d['roofline']['forward']['train']['ms'], d['roofline']['forward']['eval']['ms'])"
done
