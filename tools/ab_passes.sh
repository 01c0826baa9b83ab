#!/bin/bash
# A/B of libsketch builds on one box with the partitioned K1's per-pass times:
# ROUNDS alternations of bench.py over LIBS, extra bench args in ARGS.
O=${OUT:-bench_out}
mkdir -p $O
LIBS=${LIBS:-"tools/ab/libsketch_base.so real-time-student-attendance-system_amd/csrc/libsketch.so"}
for r in $(seq ${ROUNDS:-3}); do
  for lib in $LIBS; do
    SKE_LIB=$lib timeout -k 10 200 python bench.py --full --no-cpu --no-check $ARGS > $O/ab.log 2>&1 || { tail -5 $O/ab.log; exit 1; }
    python - "$lib" $O/ab.log <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
p = d["roofline"].get("passes", {})
print("%-48s %.4e/s  %.4f ms/step  %s" % (sys.argv[1].split("/")[-1], d["value"], d["ms_per_step"],
      " ".join("%s %.4f" % (k, v["ms"]) for k, v in p.items())))
PY
  done
done
