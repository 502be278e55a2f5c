#!/bin/bash
# Experimental library builds for A/B timing: bash tools/build_variant.sh NAME TU [extra hipcc flags...]
# recompiles csrc/TU.hip with -DTSTWO_EXPERIMENTS and the extra flags and links it with the other objects of the EXPERIMENTS
# build (python -m tstwo_amd.build --experiments; the TSTWO_* switches of DESIGN.md §8 are live in it) into build/exp/NAME.so.
# Use it through TSTWO_HIP_LIB=build/exp/NAME.so.
# TSTWO_VARIANT_SRC=DIR takes TU.hip from DIR instead of tstwo_amd/csrc: a copy of the tree's include/ and tstwo_amd/csrc/ kept
# elsewhere with one change applied (DIR = <copy>/tstwo_amd/csrc), so that a single-change variant never touches the sources here.
set -e
NAME=$1; TU=$2; shift 2
R=$(cd $(dirname $0)/.. && pwd)
SRC=${TSTWO_VARIANT_SRC:-$R/tstwo_amd/csrc}
mkdir -p $R/build/exp/obj
python3 -m tstwo_amd.build --experiments > /dev/null
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -DTSTWO_EXPERIMENTS "$@" -c $SRC/$TU.hip -o $R/build/exp/obj/${NAME}_$TU.o
OBJS=""
for s in context field_ops cfft fri merkle decommit quotients comm gkr poseidon air logup; do
  if [ $s = $TU ]; then OBJS="$OBJS $R/build/exp/obj/${NAME}_$TU.o"; else OBJS="$OBJS $R/tstwo_amd/csrc/obj/exp/$s.o"; fi
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $R/build/exp/$NAME.so $OBJS -ldl
echo built build/exp/$NAME.so
