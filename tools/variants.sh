#!/bin/bash
# Builds compile-time variants of the match kernel next to the product library (pgrc_amd/variants/, git-ignored), for
# tools/ab_libs.py to compare in one process.  Needs the product objects (make -C pgrc_amd/csrc) first.
set -eu
cd "$(dirname "$0")/.."
V=pgrc_amd/variants
declare -A DEFS=( [base]="" [vc8]="-DVC_BITS=3" [vc2]="-DVC_BITS=1" [s16]="-DMATCH_STAGE=16" [chunk256]="-DMATCH_CHUNK=256u" [vc2s16]="-DVC_BITS=1 -DMATCH_STAGE=16" )
mkdir -p $V
for v in "${!DEFS[@]}"; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Iinclude -Ipgrc_amd/csrc ${DEFS[$v]} -c pgrc_amd/csrc/copmem.hip -o $V/copmem_$v.o
  /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $V/libpgrc_match_$v.so $V/copmem_$v.o $(ls pgrc_amd/csrc/build/*.o | grep -v copmem.o)
  echo built $v
done
