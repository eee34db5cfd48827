#!/bin/bash
# builds a fake-JNI program: the JNI shim compiled against the stub jni.h (its malloc/free counted) + tests/jni_stub/<name>.c, the
# scenarios over the fake JNIEnv of fake_env.h
#   build.sh                   tests/jni_stub/fake_jni, in place
#   build.sh <name> <out-dir>  <out-dir>/<name> (tests/support.py: build_fake_jni)
set -e
here="$(cd "$(dirname "$0")" && pwd)"; root="$here/../.."
name="${1:-fake_jni}"; out="${2:-$here}"
gcc -O1 -std=gnu11 -Wall -I"$here" -I"$root/include" -Dmalloc=t_malloc -Dfree=t_free -include "$here/shim_alloc.h" -c "$root/lz4-java_amd/jni/net_jpountz_lz4_LZ4HIPJNI.c" -o "$out/shim.o"
gcc -O1 -std=gnu11 -Wall -I"$here" -I"$root/include" -c "$here/$name.c" -o "$out/$name.o"
gcc "$out/$name.o" "$out/shim.o" -L"$root/lz4-java_amd" -llz4hip -Wl,-rpath,"$root/lz4-java_amd" -Wl,-rpath,/opt/rocm/lib -o "$out/$name"
