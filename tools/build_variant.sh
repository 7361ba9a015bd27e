#!/bin/bash
# Tuning build: tools/build_variant.sh <name> [extra hipcc flags]  ->  roborugby_amd/variants/lib_<name>.so
# (only T and G in fp64, so it compiles in ~20 s; never the product library.  Lanes per arena: -DRR_TUNE_VW_T=<n> / -DRR_TUNE_VW_G=<n>,
# default the product's 2 / 8; -DRR_TUNE_VW_D=<n> adds the duel shape D, the product's is 4 -- csrc/rr_kstep.hpp)
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $ROOT/roborugby_amd/variants
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -fPIC -shared -DRR_CFG_SUBSET=1 "$@" \
  -o $ROOT/roborugby_amd/variants/lib_$NAME.so $ROOT/roborugby_amd/csrc/rr_kernels.hip $ROOT/roborugby_amd/csrc/rr_dqn.hip
echo built lib_$NAME.so
