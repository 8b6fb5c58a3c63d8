# One GPU call: the GPU test suite, then the full bench line.  Usage: bash tools/gpu_check.sh
# Test failures (rc 1) still let the bench run; a crash, abort or time limit ends the call.
# Logs go to $DG_OUT (default _out/).
set -o pipefail
O=${DG_OUT:-_out}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests/ -q --maxfail=5 --timeout 600 --timeout-method thread -m gpu > $O/pytest_gpu.log 2>&1
rc=$?
tail -1 $O/pytest_gpu.log
if [ $rc -ne 0 ]; then
  echo "TESTS rc=$rc"; grep -E "^(FAILED|ERROR)" $O/pytest_gpu.log | head -20
  [ $rc -eq 1 ] || exit $rc
fi
timeout -k 10 400 python -u bench.py --full > $O/bench.log 2>&1 || { echo BENCH_FAILED; tail -20 $O/bench.log; exit 1; }
tail -1 $O/bench.log
exit $rc
