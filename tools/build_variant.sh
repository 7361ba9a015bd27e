#!/bin/bash
# Tuning build: tools/build_variant.sh <name> [extra hipcc flags]  ->  roborugby_amd/variants/lib_<name>.so
# (only T and G in fp64, so it compiles in a few minutes; never the product library.  Lanes per arena: -DRR_TUNE_VW_T=<n> / -DRR_TUNE_VW_G=<n>,
# default the product's 2 / 8; -DRR_TUNE_VW_D=<n> adds the duel shape D, the product's is 4 -- csrc/rr_kstep.hpp)
# Every translation unit of the product library is in it (roborugby_amd/build.py): the loader resolves every symbol of the ABI.
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $ROOT/roborugby_amd/variants
CSRC=$ROOT/roborugby_amd/csrc
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -fPIC -shared -DRR_CFG_SUBSET=1 "$@" \
  -o $ROOT/roborugby_amd/variants/lib_$NAME.so $CSRC/rr_kernels.hip $CSRC/rr_dqn.hip $CSRC/rr_cnn.hip $CSRC/rr_frames.hip
echo built lib_$NAME.so
