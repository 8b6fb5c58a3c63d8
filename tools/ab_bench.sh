# A/B of a library build against the base on the bench's own numbers, alternating:
#   bash tools/ab_bench.sh <variant .so under ab/> [bench args]
# Logs go to $DG_OUT/abb (default _out/abb in the repository).
# The bench's `mutate` and `anti_entropy_hops` figures come from c_src/_build/bench_mutate and
# bench_hop, which load the in-tree library through their run path in every step: A/B those
# by running them with the variant's directory first on LD_LIBRARY_PATH.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
V=$1; shift
O=${DG_OUT:-$R/_out}/abb
mkdir -p $O
for v in base var base var; do
  if [ $v = var ]; then export DG_LIB_PATH=$R/delta_crdt_ex_amd/ab/$V; else unset DG_LIB_PATH; fi
  timeout -k 10 300 python -u $R/bench.py --full --no-cpu-baseline "$@" > $O/$v.log 2>&1 || { echo FAIL $v; tail -5 $O/$v.log; exit 1; }
  python3 - $O/$v.log $v <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith('{"metric"')][-1])
r = d["roofline"]
out = [sys.argv[2], "c2 avg_us %.2f frac %.4f" % (r["avg_launch_us"], r["frac"])]
for k in ("config5", "config3"):
    if k in d:
        out.append("%s frac %.4f us %.1f" % (k, d[k]["roofline"]["frac"], d[k]["roofline"].get("avg_launch_us", 0)))
if "merkle" in d:
    m = d["merkle"]
    out.append("build %.4f diff %.4f" % (m["roofline"]["frac"], m["diff_roofline"]["frac"]))
print(" | ".join(out))
PY
done
