#!/bin/bash
# Builds tools/bin/libgather_probe{0,1}.so (tools/gather_probe.hip with GKOMI_GATHER_PROBE = k).  Runs here: hipcc
# cross-compiles.  Also writes the kernel's ISA next to them (bin/gather_probe{0,1}.s) to check that the stand-in
# gather still waits on the column loads.
set -e
cd "$(dirname "$0")"
mkdir -p bin
for k in 0 1; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -shared --offload-arch=gfx950 -ffp-contract=off -DGKOMI_GATHER_PROBE=$k \
        gather_probe.hip -o bin/libgather_probe$k.so -L../repo-8852-ginkgo_amd/lib -lgkomi \
        '-Wl,-rpath,$ORIGIN/../../repo-8852-ginkgo_amd/lib' &
    /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -DGKOMI_GATHER_PROBE=$k \
        --cuda-device-only -S gather_probe.hip -o bin/gather_probe$k.s &
done
wait
ls -la bin/libgather_probe*.so
