#!/bin/bash
# Are the results of two product libraries the same?  tools/dumps_equal.sh <out.txt> <workdir> <libA.so> <libB.so> -- "<bench args>" ...
# Runs `bench.py --arenas 4096 --steps 20 --warmup 10 --dump-outputs` with each library (RR_LIB_PATH) and compares every dumped array
# with numpy.array_equal, NaN-strict.  One line per set of arguments; exit code 1 if anything differs or a run fails.
OUT=$1; WORK=$2; LIBA=$(readlink -f $3); LIBB=$(readlink -f $4); shift 5
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$(dirname $OUT)" $WORK; : > $OUT; bad=0; k=0
for ARGS in "$@"; do
  k=$((k + 1))
  for side in a b; do
    lib=$LIBA; [ $side = b ] && lib=$LIBB
    RR_LIB_PATH=$lib timeout -k 10 300 python3 $ROOT/bench.py --gpus 1 --arenas 4096 --steps 20 --warmup 10 $ARGS --dump-outputs $WORK/$k$side > $WORK/$k$side.json 2> $WORK/$k$side.err \
      || { echo "run failed: $ARGS ($lib)"; tail -5 $WORK/$k$side.err; exit 1; }
  done
  python3 - "$ARGS" $WORK/${k}a $WORK/${k}b <<'PY' | tee -a $OUT
import glob, os, sys
import numpy as np
args, a, b = sys.argv[1:]
names = sorted(os.path.basename(f)[:-4] for f in glob.glob(a + "/*.npy"))
assert names and names == sorted(os.path.basename(f)[:-4] for f in glob.glob(b + "/*.npy")), (a, b)
diff = [n for n in names if not np.array_equal(np.load(f"{a}/{n}.npy"), np.load(f"{b}/{n}.npy"), equal_nan=True)]
strict = [n for n in names if not np.array_equal(np.load(f"{a}/{n}.npy"), np.load(f"{b}/{n}.npy"))]
print("%-28s %d arrays (%s): %s; NaN-strict numpy.array_equal differs in: %s" % (args or "(headline)", len(names), " ".join(names),
      "ALL EQUAL" if not diff else "DIFFER: " + " ".join(diff), " ".join(strict) or "none"))
sys.exit(1 if diff else 0)
PY
  [ ${PIPESTATUS[0]} -ne 0 ] && bad=1
done
exit $bad
