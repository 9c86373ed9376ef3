#!/bin/bash
# Builds the C-ABI library of another revision next to the working tree's, for same-box A/B runs (bench.py --lib <dir>/liblang2seg_hip.so):
#   tools/ab_build.sh <git rev> [output dir]     (default build/ab_<rev>; the Python host stays the working tree's; only the kernels differ)
# The compile flags are the product build's (__graft_entry__.HIPCC_FLAGS of the working tree), so the two libraries differ in their sources only.
set -e
REV=${1:-HEAD}
R=$(cd "$(dirname "$0")/.." && pwd)
D=${2:-$R/build/ab_$REV}
rm -rf "$D"; mkdir -p "$D"
D=$(cd "$D" && pwd)
git -C "$R" archive "$REV" lang2seg_amd/csrc include | tar -x -C "$D"
FLAGS=$(cd "$R" && python -c "import shlex; from __graft_entry__ import HIPCC_FLAGS; print(' '.join(shlex.quote(f) for f in HIPCC_FLAGS))")
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
cd "$D"
ls lang2seg_amd/csrc/*.hip | xargs -P 6 -I{} sh -c "$HIPCC $FLAGS -c {} -o \$(basename {} .hip).o"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o liblang2seg_hip.so *.o
rm -f *.o
ls -la "$D/liblang2seg_hip.so"
