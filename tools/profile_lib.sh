#!/bin/bash
# k_step's time and SQ counters for one product library on the headline command: tools/profile_lib.sh <outdir> <lib.so>
# Two separate rocprofv3 processes (a kernel trace with statistics; the counters alone), then one summary:
# <outdir>/summary.txt -- k_step's mean over the timed launches, and VALU / SALU instructions and wave cycles per wavefront-step.
OUTD=$1; LIB=$(readlink -f $2)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $OUTD; OUTD=$(readlink -f $OUTD)
export RR_LIB_PATH=$LIB
STEPS=200
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUTD/trace -- python3 $ROOT/bench.py --gpus 1 --steps $STEPS --warmup 20 > $OUTD/trace.txt 2>&1 \
  || { echo "trace run failed"; tail -5 $OUTD/trace.txt; exit 1; }
timeout -k 10 400 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY --output-format csv -d $OUTD/pmc \
  -- python3 $ROOT/bench.py --gpus 1 --steps 20 --warmup 5 > $OUTD/pmc.txt 2>&1 || { echo "counter run failed"; tail -5 $OUTD/pmc.txt; exit 1; }
python3 - $OUTD $STEPS "${LIB#$ROOT/}" <<'PY' | tee $OUTD/summary.txt
import collections, csv, glob, sys
outd, steps, tag = sys.argv[1], int(sys.argv[2]), sys.argv[3]
rows = [r for f in glob.glob(outd + "/trace/**/*_kernel_trace.csv", recursive=True) for r in csv.DictReader(open(f)) if "k_step" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows[-steps:]]
print(f"{tag}: k_step launches {len(rows)}, timed region (last {len(d)}): avg {sum(d) / len(d):.4f} ms min {min(d):.4f} max {max(d):.4f}")
acc = collections.defaultdict(list)
for f in glob.glob(outd + "/pmc/**/*_counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "k_step" in r["Kernel_Name"]:
            acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
c = {k: sum(v[-20:]) / len(v[-20:]) for k, v in acc.items()}  # the timed launches of the counter run
w = c["SQ_WAVES"]
print(f"{tag}: per wavefront-step: " + " ".join(f"{k} {c[k] / w:.0f}" for k in sorted(c) if k != "SQ_WAVES") + f" (SQ_WAVES {w:.0f})")
print(f"{tag}: VALU active / wave cycles {c['SQ_ACTIVE_INST_VALU'] / c['SQ_WAVE_CYCLES']:.4f}  wait_any / wave cycles {c['SQ_WAIT_ANY'] / c['SQ_WAVE_CYCLES']:.4f}")
PY
