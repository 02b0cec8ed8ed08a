#!/bin/bash
# Debug build of libmpcq.so (dev tool; needs the regular build's objects): the host files (mpcq_host_*.cpp) and one kernel
# source (default mpcq_tile_f32.hip; SRC=... to pick another) recompiled with -DMPCQ_DEBUG_HOOKS (the
# stamp / profiling dumps, mpcq_ctx.h "Test hooks") plus the extra defines given.
# usage: [SRC=mpcq_mimo.hip] bash tools/build_dbg.sh [MPCQ_INFO_STAMPS ...]  ->  tools/dbglib/libmpcq.so
#        then MPCQ_LIBRARY=tools/dbglib/libmpcq.so MPCQ_TILE_STAMPS=out.bin python ...
set -e
cd "$(dirname "$0")/../solvempc_amd/csrc"
D=../../${DBGDIR:-tools/dbglib}; mkdir -p $D
SRC=${SRC:-mpcq_tile_f32.hip}
DEFS="-DMPCQ_DEBUG_HOOKS $(for d in "$@"; do printf -- "-D%s " "$d"; done)"
FL="-O3 -ffp-contract=off -fno-slp-vectorize -std=c++17 -fPIC --offload-arch=gfx950"
/opt/rocm/bin/hipcc $FL $DEFS -c $SRC -o $D/dbg_src.o
host=""
for f in mpcq_host_*.cpp; do
  /opt/rocm/bin/hipcc $FL $DEFS -c $f -o $D/dbg_${f%.cpp}.o
  host="$host $D/dbg_${f%.cpp}.o"
done
objs=$(ls build/*.o | grep -v -e "$SRC" -e mpcq_host_)
/opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o $D/libmpcq.so $objs $D/dbg_src.o $host
