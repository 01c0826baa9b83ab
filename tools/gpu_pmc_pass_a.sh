#!/bin/bash
# Pass A's issue and wait counters over the default C3 bench (2^28 swipes per
# step, sub-batches of 2^25), as tools/gpu_pmc_seg.sh collects them: one
# counter group per rocprofv3 run, --pmc only.  The summary of k_part_a3 goes
# to $OUT/pmc_<ROUND>_k_part_a.json (tools/pmc_summary.py; the two warm-up
# steps' 16 dispatches skipped).  SKE_LIB picks an A/B build.
# usage: ROUND=r07 OUT=bench_out bash tools/gpu_pmc_pass_a.sh [extra bench args]
ARGS="--steps 4 --warmup 2 --no-cpu --no-check --secondary none --pass-replay 0 --host-fed 0 $*"
R=${ROUND:-r07}
O=${OUT:-bench_out}
mkdir -p $O/pmc_$R
export TMPDIR=/tmp
GROUPS_=("SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY" "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_LDS"
 "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE")
for c in "${GROUPS_[@]}"; do
  tag=$(echo $c | tr ' ' '_')
  timeout -s KILL 240 rocprofv3 --pmc $c -d $O/pmc_$R/$tag -o run --output-format csv -- python bench.py $ARGS > $O/pmc_$R/$tag.log 2>&1; rc=$?
  echo "pmc [$c] rc=$rc"
  if [ $rc -ne 0 ]; then tail -3 $O/pmc_$R/$tag.log; exit $rc; fi
done
python tools/pmc_summary.py $O/pmc_$R k_part_a3 $O/pmc_${R}_k_part_a.json 16 || exit 1
