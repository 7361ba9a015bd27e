#!/bin/bash
# A/B lanes per arena: tools/ab_vw.sh "<bench args>" <T|G|D> vw1 vw2 ...
# One tuning build per width (tools/build_variant.sh -DRR_TUNE_VW_<shape>=<vw>: fp64 only, the other shapes at the product's widths),
# then tools/ab.sh over them through RR_LIB_PATH.  Build on the box that has hipcc; give the shape's own --preset in <bench args>.
set -e
ARGS="$1"; SHAPE="$2"; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
LIBS=""
for vw in "$@"; do
  bash $ROOT/tools/build_variant.sh vw_${SHAPE}$vw -DRR_TUNE_VW_$SHAPE=$vw
  LIBS="$LIBS $ROOT/roborugby_amd/variants/lib_vw_${SHAPE}$vw.so"
done
cd $ROOT && bash tools/ab.sh "$ARGS" $LIBS
