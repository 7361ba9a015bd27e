#!/bin/bash
# A/B of bench.py lines between product libraries, alternating: tools/ab_lines.sh <out.txt> <reps> <libA.so> <libB.so> -- "<bench args>" ...
# Every run: its own process under its own time limit, selected with RR_LIB_PATH.  The script stops at the first run whose bench process
# does not exit with 0 (an abort, a fault or the time limit included, whatever it printed) or prints no result line: nothing more is started.
# One output line per run: bench arguments, repetition, library, env-steps/s, mean k_step time per launch.
OUT=$1; REPS=$2; LIBA=$(readlink -f $3); LIBB=$(readlink -f $4); shift 5
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$(dirname $OUT)"; : > $OUT
for ARGS in "$@"; do
  for rep in $(seq 1 $REPS); do
    for lib in $LIBA $LIBB; do
      RR_LIB_PATH=$lib timeout -k 10 300 python3 $ROOT/bench.py --gpus 1 $ARGS > $OUT.run 2> $OUT.err; rc=$?
      if [ $rc -ne 0 ]; then echo "run failed with exit code $rc: $ARGS ($lib)"; tail -5 $OUT.err; exit 1; fi
      line=$(python3 -c "
import sys, json
for l in open(sys.argv[1]):
    try: d = json.loads(l)
    except Exception: continue
    print('%10.4f M env-steps/s kernel_ms %.4f' % (d['value'] / 1e6, d['roofline']['kernel_ms']))
" $OUT.run)
      if [ -z "$line" ]; then echo "no result line: $ARGS ($lib)"; tail -5 $OUT.err; exit 1; fi
      printf "%-52s rep %d %-62s %s\n" "$ARGS" $rep "${lib#$ROOT/}" "$line" | tee -a $OUT
    done
  done
done
rm -f $OUT.err $OUT.run
