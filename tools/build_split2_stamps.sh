#!/bin/bash
# build/ab/split2_stamps.so = the library with gru_split2.o rebuilt with -DDGRP_SPLIT2_STAMPS: the DIAGNOSTIC build whose workgroups
# write clock stamps at the boundaries of every tile pair (gru_split2.hip; read by tools/split2_stamps.py).  Never the product build.
# Built like the Makefile builds the object (same flags, the ISA audit on the compiler's output), the other objects as they are.
set -e
cd "$(dirname "$0")/../deepgrp_amd/csrc"
make -s all
out=../../build/ab/split2_stamps
rm -rf $out && mkdir -p $out
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -fPIC -fvisibility=hidden -std=c++17 -Wall -Wno-unused-function -fno-slp-vectorize \
    -DDGRP_SPLIT2_STAMPS -save-temps=obj -c gru_split2.hip -o $out/gru_split2.o
# (the stamps' addresses cost a few scalar registers at the pair boundaries: the allocator parks 6 of them in lanes of a vector register
# OUTSIDE the time loop, whose instruction mix stays that of the product -- the audit's other findings, hazards and scratch, still fail)
DGRP_LINT_ALLOW_SCRATCH=1 python3 ../../tools/lint_split2_isa.py $out/gru_split2-hip-amdgcn-amd-amdhsa-gfx950.s > $out/lint.txt || (cat $out/lint.txt; false)
if grep -E "private_segment_fixed_size: +[1-9]|vgpr_spill_count: +[1-9]" $out/gru_split2-hip-amdgcn-amd-amdhsa-gfx950.s; then echo "scratch in the diagnostic build"; exit 1; fi
objs=""
for o in $(sed -n 's/^OBJS *:= *//p' Makefile); do
    if [ $o = gru_split2.o ]; then objs="$objs $out/$o"; else objs="$objs $o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out.so $objs
rm -rf $out
echo "built build/ab/split2_stamps.so"
