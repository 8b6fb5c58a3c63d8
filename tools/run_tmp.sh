# A/B of the in-tree library against ab/libdeltagpu_base.so: the Merkle / join_delta tests,
# the bench's config-4 round twice each (alternating), then that round under rocprofv3.
# Everything goes to $DG_OUT/t (default _out/t in the repository).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd $R
O=${DG_OUT:-$R/_out}/t
mkdir -p $O && O=$(cd $O && pwd)
timeout -k 10 600 python -u -m pytest -x -q --timeout 300 --timeout-method thread tests/test_gpu_merkle.py tests/test_gpu_binding.py tests/test_gpu_join_delta.py tests/test_gpu_configs.py tests/test_gpu_splice.py -m gpu > $O/tests.log 2>&1 || { echo TEST_FAIL; tail -30 $O/tests.log; exit 1; }
tail -1 $O/tests.log
for round in 1 2; do for v in base intree; do
  if [ $v = intree ]; then unset DG_LIB_PATH DG_LIB_ANY_DIGEST; else export DG_LIB_PATH=$R/delta_crdt_ex_amd/ab/libdeltagpu_$v.so DG_LIB_ANY_DIGEST=1; fi
  timeout -k 10 300 python -u bench.py --full --no-configs --no-cpu-baseline --steps 20 --warmup 5 > $O/b_$v$round.log 2>&1 || { echo BENCH_FAIL; tail -5 $O/b_$v$round.log; exit 1; }
  python3 - $O/b_$v$round.log $v <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith('{"metric"')][-1])
m = d["merkle"]
print(sys.argv[2], "join_delta wall %.1f dev %.1f | diff %.1f take %.1f | c2 frac %.4f" % (m["round_us"]["join_delta"], m["join_delta_device_us"], m["round_us"]["diff"], m["round_us"]["take"], d["roofline"]["frac"]))
PY
done; done
unset DG_LIB_PATH DG_LIB_ANY_DIGEST
cd /tmp && export TMPDIR=/tmp
for v in base intree; do
  if [ $v = intree ]; then unset DG_LIB_PATH DG_LIB_ANY_DIGEST; else export DG_LIB_PATH=$R/delta_crdt_ex_amd/ab/libdeltagpu_$v.so DG_LIB_ANY_DIGEST=1; fi
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/mk_$v -o mk -- python3 $R/tools/prof_merkle.py > $O/mk_$v.log 2>&1 || { echo MK_FAIL; tail -5 $O/mk_$v.log; exit 1; }
  echo "== $v"; python3 $R/tools/kernel_timeline.py $O/mk_$v 6 | tail -7
done
rm -f $O/*/*kernel_trace.csv
