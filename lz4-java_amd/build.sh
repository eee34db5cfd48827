#!/bin/bash
# Builds lz4-java_amd/liblz4hip.so for gfx950 (cross-compiles without a GPU): every csrc/*.hip unit and api.cpp to an object of its
# own, side by side, then one link.  Always everything, into a fresh object directory that is removed afterwards: no stale objects.
#   LZ4HIP_OUT          the library to write (default: liblz4hip.so next to this script)
#   LZ4HIP_EXTRA_FLAGS  further compile flags (developer builds: tools/build_variant.sh)
#   MAX_JOBS            compile jobs at a time (default and most: 16)
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
out="${LZ4HIP_OUT:-$here/liblz4hip.so}"
jobs="${MAX_JOBS:-16}"
if [ "$jobs" -gt 16 ]; then jobs=16; fi
if [ "$jobs" -lt 1 ]; then jobs=1; fi
mkdir -p "$here/build"
obj="$(mktemp -d "$here/build/obj.XXXXXX")"
trap 'rm -rf "$obj"' EXIT
# (-mllvm -structurizecfg-skip-uniform-regions=1 is worth +3 % on fast compress and MISCOMPILES the long-buffer xxhash kernels:
# block checksums came out wrong in tests/test_gpu_streams.py -- do not use it)
compile() {
  "$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 ${LZ4HIP_EXTRA_FLAGS:-} -fPIC -fvisibility=hidden -c "$1" -o "$2"
}
objs=()
running=0
failed=0
for src in "$here"/csrc/*.hip "$here/csrc/api.cpp"; do
  o="$obj/$(basename "$src").o"
  objs+=("$o")
  if [ "$running" -ge "$jobs" ]; then wait -n || failed=1; running=$((running - 1)); fi
  compile "$src" "$o" &
  running=$((running + 1))
done
while [ "$running" -gt 0 ]; do wait -n || failed=1; running=$((running - 1)); done
if [ "$failed" -ne 0 ]; then echo "build.sh: a unit failed to compile" >&2; exit 1; fi
"$HIPCC" --offload-arch=gfx950 -fPIC -shared -fvisibility=hidden -Wl,-rpath,/opt/rocm/lib -Wl,--exclude-libs,ALL "${objs[@]}" -o "$out"
echo "built $out"
