# A/B builds of jh_lin.hip: tools/build_variants.sh name "-DFLAG ..." [name "flags"]...
# Each variant links its own jh_lin.o with the release build's other objects
# (the objects of build.py's source lists: a stale one left in build/ is not linked).
set -e
cd "$(dirname "$0")/.."
others=$(python -c "
import os
from jepsen_amd import build as B
B.build_libjh()
print(' '.join(os.path.join(B.OBJ, os.path.splitext(s)[0] + '.o') for s in B.HIP_SOURCES + B.HOST_SOURCES if s != 'jh_lin.hip'))")
mkdir -p jepsen_amd/variants
while [ $# -ge 2 ]; do
  n=$1; f=$2; shift 2
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $f -c jepsen_amd/csrc/jh_lin.hip -o /tmp/jh_lin_$n.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o jepsen_amd/variants/libjh_$n.so /tmp/jh_lin_$n.o $others -pthread
done
