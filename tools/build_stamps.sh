#!/bin/bash
# Development only: builds an instrumented copy of the library (per-stage cycle stamps in the resident decode kernel)
# into tools/_stamps/libeamrl_hip.so; use with EAMRL_HIP_LIB=tools/_stamps/libeamrl_hip.so python tools/stamps.py
# The sources and compiler flags are those of eam_rl4co_amd/build.py, plus -DEAMRL_STAMPS.
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/_stamps
SOURCES=$(python -c "from eam_rl4co_amd.build import SOURCES; print(' '.join(SOURCES))")
FLAGS="$(python -c "from eam_rl4co_amd.build import FLAGS; print(' '.join(FLAGS))") -DEAMRL_STAMPS"
for f in $SOURCES; do
  /opt/rocm/bin/hipcc $FLAGS -c eam_rl4co_amd/csrc/$f -o tools/_stamps/${f%.hip}.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/_stamps/libeamrl_hip.so tools/_stamps/*.o
rm -f tools/_stamps/*.o
echo built tools/_stamps/libeamrl_hip.so
