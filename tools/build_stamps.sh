#!/bin/bash
# Diagnostic build with per-phase s_memtime stamps (tools/stamps.py reads them).
# One translation unit: the stamp counters are one device symbol.
#   bash tools/build_stamps.sh [out.so] [extra hipcc flags, e.g. -DBIOIM_GROUND_ONCE=0]
set -e
cd "$(dirname "$0")/.."
C=bioimitation-gym_amd/csrc
out=${1:-bioimitation-gym_amd/build/libbioim_stamps.so}
[ $# -gt 0 ] && shift
# the shipped library's flags (bioimitation/_buildinfo.py: one place for them)
FLAGS=$(cd bioimitation-gym_amd && python3 -m bioimitation._buildinfo flags)
mkdir -p "$(dirname "$out")"
hipcc $FLAGS -shared -DBIOIM_STAMPS "$@" -o "$out" $C/bioim_step.hip
