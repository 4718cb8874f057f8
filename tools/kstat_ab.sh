#!/bin/bash
# GPU side: per-kernel average durations (rocprofv3 --kernel-trace --stats) of the C2 stream for
# prebuilt variants (tools/variants.sh): bash tools/kstat_ab.sh NAME... Prints the ICP loop's
# kernels; the full tables stay under gpurun_out/kab_NAME/.
# Another workload, other kernels, or a name given more than once (new parent parent new):
#   ARGS  bench.py arguments;  KEYS  kernel name parts to print;  TAG  suffix of the table
#   directories (kab_NAME_TAG_RUN), without which a repeated name keeps its last run only.
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
ARGS=${ARGS:---steps 5 --warmup 1 --no-cpu-baseline --no-batched}
KEYS=${KEYS:-k_icp_nn k_sel_ k_icp_reduce k_icp_update k_knn_oct k_tr_mid k_ovl_mark}
mkdir -p gpurun_out
i=0
for v in "$@"; do
  i=$((i + 1))
  OUT=gpurun_out/kab_$v
  [ -n "$TAG" ] && OUT=${OUT}_${TAG}_$i
  rm -rf $OUT && mkdir -p $OUT
  AICP_HIP_LIB=$PWD/build_ab/lib_$v.so timeout -k 10 280 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o run -- python3 bench.py $ARGS > $OUT/bench.log 2>&1 || { tail -20 $OUT/bench.log; exit 1; }
  echo "== $v"
  python3 - "$(find $OUT/trace -name '*kernel_stats.csv' | head -1)" $KEYS <<'PY' || exit 1
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    n = r["Name"].replace("(anonymous namespace)::", "")
    if any(k in n for k in sys.argv[2:]):
        print("%-28s %6s %9.2f us" % (n.split("(")[0][-28:], r["Calls"], float(r["AverageNs"]) / 1e3))
PY
done
