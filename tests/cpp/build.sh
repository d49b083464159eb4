#!/bin/bash
# Builds the C++ host-API test binary (g++; links the product library and, as the checker, the oracle).
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"; ROOT="$(cd "$HERE/../.." && pwd)"
mkdir -p "$HERE/bin"
for t in test_icp test_model_estimation; do
g++ -O2 -std=c++17 -ffp-contract=off -I"$ROOT/include" "$HERE/$t.cpp" -o "$HERE/bin/$t" \
    -L"$ROOT/cilantro_amd/lib" -lcilantro_hip -L"$ROOT/oracle" -loracle \
    -Wl,-rpath,"$ROOT/cilantro_amd/lib" -Wl,-rpath,"$ROOT/oracle" -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64
done
# host-side check of the fast paths in csrc/solve.hpp (hipcc: the header pulls in the HIP runtime API; runs without a GPU)
/opt/rocm/bin/hipcc -O2 -std=c++17 -ffp-contract=off --offload-arch=gfx950 "$HERE/test_solve.cpp" -o "$HERE/bin/test_solve"
# host-only check of the ICP loops' form policy (csrc/loop_policy.hpp: plain C++, no HIP)
g++ -O2 -std=c++17 -Wall -ffp-contract=off "$HERE/test_loop_policy.cpp" -o "$HERE/bin/test_loop_policy"
# host-only check of the grid's shape policy (csrc/grid_policy.hpp: plain C++, no HIP)
g++ -O2 -std=c++17 -Wall -ffp-contract=off "$HERE/test_grid_policy.cpp" -o "$HERE/bin/test_grid_policy"
# host-only check of the owners of device allocations (csrc/device_mem.hpp over a counting malloc allocator: plain C++, no HIP)
g++ -O2 -std=c++17 -Wall -ffp-contract=off "$HERE/test_device_mem.cpp" -o "$HERE/bin/test_device_mem"
# host-only check of the RANSAC estimators' sampler (csrc/ransac_sampling.hpp: plain C++, no HIP) against a copy of the loop it replaced
g++ -O2 -std=c++17 -Wall -ffp-contract=off "$HERE/test_ransac_sampling.cpp" -o "$HERE/bin/test_ransac_sampling"
# tests/cpp/tie_order_host.hpp (the host restatement of the reference's index build: the cross-check of csrc/tie_build.hip) as a host library
g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -pthread "$HERE/tie_order_shim.cpp" -o "$HERE/bin/libtie_order_shim.so"
# host-only PLY round-trip helper (no GPU library needed)
g++ -O2 -std=c++17 -I"$ROOT/include" "$HERE/test_ply.cpp" -o "$HERE/bin/test_ply"
# the example program (compile check; run it on a GPU box with a PLY file)
g++ -O2 -std=c++17 -I"$ROOT/include" "$ROOT/examples/rigid_icp.cpp" -o "$HERE/bin/example_rigid_icp" \
    -L"$ROOT/cilantro_amd/lib" -lcilantro_hip -Wl,-rpath,"$ROOT/cilantro_amd/lib" -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64
# host-only sweep of the option table (csrc/ctx_options.hpp behind cilhip_set_option / cilhip_get_option: a context constructed on the host
# takes both without a device), once plainly and once under the address and undefined-behaviour sanitizers (hipcc: ctx.hpp pulls in the HIP runtime API)
for v in "" "_san"; do
SAN=""; [ -n "$v" ] && SAN="-g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all"
/opt/rocm/bin/hipcc -O1 -std=c++17 -ffp-contract=off --offload-arch=gfx950 $SAN "$HERE/test_ctx_options.cpp" -o "$HERE/bin/test_ctx_options$v" \
    -L"$ROOT/cilantro_amd/lib" -lcilantro_hip -Wl,-rpath,"$ROOT/cilantro_amd/lib" -Wl,-rpath,/opt/rocm/lib
done
