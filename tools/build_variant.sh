#!/bin/bash
# usage: tools/build_variant.sh <name> [extra hipcc flags...]  -> lz4-java_amd/variants/<name>.so (developer A/B builds, git-ignored)
# The compile recipe is lz4-java_amd/build.sh's; this only names the output and passes the flags on.
set -euo pipefail
here="$(cd "$(dirname "$0")/.." && pwd)"
name=$1; shift
mkdir -p "$here/lz4-java_amd/variants"
LZ4HIP_OUT="$here/lz4-java_amd/variants/$name.so" LZ4HIP_EXTRA_FLAGS="$*" exec bash "$here/lz4-java_amd/build.sh"
