#!/bin/bash
# usage: tools/resources.sh [out.txt [objdir]] -- kernel-resource-usage remarks of the three units of the fused objective (csrc/cmax_event_launch.hip,
# csrc/cmax_batch.hip, csrc/cmax_fused.hip; device-only compiles, appended to the one output file), see tools/kernel_resources.py; with objdir the device
# objects are kept there as <unit>.o (tools/head_listing.py disassembles them)
out=${1:-/tmp/res.txt}
objdir=${2:-}
: > "$out"
for unit in cmax_event_launch cmax_batch cmax_fused; do
  obj=/tmp/x.o
  [ -n "$objdir" ] && mkdir -p "$objdir" && obj="$objdir/$unit.o"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -fno-gpu-rdc -mllvm -amdgpu-kernarg-preload-count=16 --cuda-device-only -c \
    event_based_optical_flow_amd/csrc/$unit.hip -o "$obj" -Rpass-analysis=kernel-resource-usage $CMAX_EXTRA_FLAGS 2>> "$out"
done
