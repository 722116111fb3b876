#!/bin/bash
# Development only: builds a copy of the library with extra -D flags into tools/_variants/<name>/libeamrl_hip.so, for
# A/B measurements inside one gpurun call (EAMRL_HIP_LIB=tools/_variants/<name>/libeamrl_hip.so python bench.py ...).
#   usage: bash tools/build_variant.sh du5_4 -DEAMRL_DU5=4
# The sources and compiler flags are those of eam_rl4co_amd/build.py, plus the extra flags.
set -e
cd "$(dirname "$0")/.."
NAME=$1; shift
D=tools/_variants/$NAME
mkdir -p $D
SOURCES=$(python -c "from eam_rl4co_amd.build import SOURCES; print(' '.join(SOURCES))")
FLAGS="$(python -c "from eam_rl4co_amd.build import FLAGS; print(' '.join(FLAGS))") $*"
for f in $SOURCES; do
  /opt/rocm/bin/hipcc $FLAGS -c eam_rl4co_amd/csrc/$f -o $D/${f%.hip}.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $D/libeamrl_hip.so $D/*.o
rm -f $D/*.o
echo built $D/libeamrl_hip.so
