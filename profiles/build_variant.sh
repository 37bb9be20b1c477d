#!/bin/bash
# Experimental build of the kernels into libacm_amd/lib/exp/<name>.so (travels to the GPU box; *.so is git-ignored):
#   profiles/build_variant.sh <name> [-DFLAG ...]          (the other objects are the regular build's)
# The flags go to the kernels AND to acm_kernel_geo.cpp, the planner's view of their geometry: a flag that changes a tile
# (ACM_K3_DPP_HISTORY, ACM_K3_L13_TILE, ACM_K2M_L1x_TILE ...) must reach both, or acmhip_device_open refuses the library.
# A/B on the box: python3 profiles/ab_kernels.py libacm_amd/lib/libacm_hip.so libacm_amd/lib/exp/<name>.so ...
set -e
cd "$(dirname "$0")/.."
NAME=$1; shift
SRC=${ACM_KERNEL_SRC:-libacm_amd/csrc/acm_kernels.hip}
python3 -c "from libacm_amd import _build; _build.build_hip()"
mkdir -p libacm_amd/lib/exp
hipcc -O3 -g1 -std=c++17 -fPIC -Wall -Wextra --offload-arch=gfx950 -I include -I libacm_amd/csrc "$@" -c $SRC -o libacm_amd/lib/exp/$NAME.kernels.o
g++ -O3 -g1 -std=c++17 -fPIC -Wall -Wextra -I include -I libacm_amd/csrc "$@" -c libacm_amd/csrc/acm_kernel_geo.cpp -o libacm_amd/lib/exp/$NAME.geo.o
# every regular object except the two rebuilt here
OBJS=$(ls libacm_amd/lib/*.o | grep -v -e '/acm_kernels\.hip\.o$' -e '/acm_kernel_geo\.cpp\.o$')
hipcc -shared -fPIC --offload-arch=gfx950 -o libacm_amd/lib/exp/$NAME.so libacm_amd/lib/exp/$NAME.kernels.o libacm_amd/lib/exp/$NAME.geo.o $OBJS -lpthread
rm -f libacm_amd/lib/exp/$NAME.kernels.o libacm_amd/lib/exp/$NAME.geo.o
ls -la libacm_amd/lib/exp/$NAME.so
