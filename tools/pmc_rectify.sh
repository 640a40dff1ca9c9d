#!/bin/bash
# PMC passes (<= 3 counters each, nothing traced beside them) over the image rectifier's kernel; usage on a machine with an MI355X:
#   bash tools/pmc_rectify.sh [pairs] [variant a|b] [output directory]
# prints every counter summed over the launches of the pass and per launch
set -u
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
B=${1:-1024}
VARIANT=${2:-b}
OUT=${3:-$R/build/pmc_rectify}
mkdir -p $OUT && OUT=$(cd $OUT && pwd)
rm -rf $OUT/p[0-9]*
cd /tmp && export TMPDIR=/tmp
i=0
for set in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY" "SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS" \
           "SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU" "SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS" \
           "SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_VMEM" "GRBM_GUI_ACTIVE TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum"; do
  i=$((i+1))
  timeout -k 10 200 rocprofv3 --pmc $set --output-format csv -d $OUT/p$i -- python3 $R/tools/bench_rectify.py $B --variant $VARIANT \
      --rounds 1 --no-host > $OUT/p$i.log 2>&1
  rc=$?
  echo "pass $i ($set) rc=$rc"
  if [ $rc -ne 0 ]; then tail -5 $OUT/p$i.log; exit 1; fi
done
python3 - <<PY
import csv,glob,collections
acc=collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob("$OUT/p*/*/*_counter_collection.csv"):
    for r in csv.DictReader(open(f)):
        k=r["Kernel_Name"]
        if "rectify_kernel" in k: acc[k.split("(")[0][-60:]][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k,d in acc.items():
    print(k)
    for c,v in sorted(d.items()): print("   %-24s %16.0f total over %d launches, %12.0f per launch" % (c, sum(v), len(v), sum(v)/len(v)))
PY
