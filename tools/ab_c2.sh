# Config-2 join A/B of several library builds (the driver's bench settings; --full with
# configs, Merkle and CPU baseline off: the headline plus its per-step event pass),
# alternating, two rounds:  bash tools/ab_c2.sh <variant .so under ab/>...
# Logs go to $DG_OUT/abc2 (default _out/abc2 in the repository).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
export DG_LIB_ANY_DIGEST=1
O=${DG_OUT:-$R/_out}/abc2
mkdir -p $O
for round in $(seq 1 ${ROUNDS:-2}); do
  for v in intree "$@"; do
    if [ $v = intree ]; then unset DG_LIB_PATH; else export DG_LIB_PATH=$R/delta_crdt_ex_amd/ab/$v; fi
    timeout -k 10 300 python -u $R/bench.py --full --no-cpu-baseline --no-merkle --no-configs --steps 20 --warmup 5 > $O/$v.log 2>&1 || { echo FAIL $v; tail -5 $O/$v.log; exit 1; }
    python3 -c "
import json,sys
d=json.loads([l for l in open('$O/$v.log') if l.startswith('{\"metric\"')][-1])
r=d['roofline']; print('$v', 'c2 avg_us %.2f frac %.4f step_med %.2f' % (r['avg_launch_us'], r['frac'], r['per_step_event_median_us']))"
  done
done
