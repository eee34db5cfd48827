"""No-GPU checks of the mirrors of the many-container write call: the C++ host mirror builds (-Werror) and runs its argument-error
scenarios; the JNI natives are declared, used and defined, the shim type-checks, and over the fake JNIEnv NULL and short arrays are
argument errors, the bound native needs no device, malloc / free balance, and without a device the write fails loudly."""
import os
import re
import subprocess

from conftest import ROOT
from support import build_fake_jni, build_mirror, no_device, typecheck_jni_shim


def test_cpp_mirror_write_many_builds_and_runs_its_argument_errors(tmp_path):
    exe = build_mirror("container_write_many_mirror_test", tmp_path, werror=True)
    out = subprocess.check_output([exe, "--args"]).decode()
    assert "checks ok" in out, out
    if no_device():
        assert "call failed" in out and "no HIP device" in out, out
        (tmp_path / "p.bin").write_bytes(b"\x01\0\0\0" + b"\x05\0\0\0\0\0\0\0hello")
        for mode in (["0", "4", "0x1c"], ["1", "64", "0"]):
            p = subprocess.run([exe, "--streams"] + mode + [str(tmp_path / "p.bin"), str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert p.returncode == 3 and b"no HIP device" in p.stderr, (mode, p.returncode, p.stdout, p.stderr)
    else:
        assert "call ok" in out, out


def test_jni_write_many_natives_declared_and_checked_without_device(tmp_path):
    jdir = os.path.join(ROOT, "lz4-java_amd", "java", "net", "jpountz", "lz4")
    java = open(os.path.join(jdir, "LZ4HIPJNI.java")).read()
    batch = open(os.path.join(jdir, "LZ4HIPBatch.java")).read()
    shim = open(os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")).read()
    assert re.search(r"static native int LZ4HIP_containerBlocksMany\(int kind, int level, ByteBuffer src, long\[\] srcOff, long\[\] srcLen, int\[\] blockSize, "
                     r"int\[\] flags,\s+int\[\] gapHead, int\[\] gapTail, int nItems, ByteBuffer dest, long destOff, long destCap, long\[\] itemDstOff, "
                     r"int\[\] contentHash\);", java)
    assert re.search(r"static native int LZ4HIP_containerBlocksManyBound\(int kind, long\[\] srcLen, int\[\] blockSize, int\[\] flags, int\[\] gapHead, "
                     r"int\[\] gapTail,\s+int nItems, int\[\] itemBlocks, long\[\] itemDstBytes\);", java)
    # the existing native keeps its signature
    assert re.search(r"static native \w+ LZ4HIP_containerBlocks\(int kind, int flags, int level,", java)
    assert "LZ4HIPJNI.LZ4HIP_containerBlocksMany(" in batch and "LZ4HIPJNI.LZ4HIP_containerBlocksManyBound(" in batch
    assert re.search(r"public static void containerBlocksMany\(int kind, int level, ByteBuffer src,", batch)
    assert re.search(r"public static void containerBlocksManyBound\(int kind, long\[\] srcLen,", batch)
    assert "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerBlocksMany(" in shim and "Java_net_jpountz_lz4_LZ4HIPJNI_LZ4HIP_1containerBlocksManyBound(" in shim
    typecheck_jni_shim()
    exe = build_fake_jni("fake_jni_container_write_many", tmp_path)
    if no_device():
        out = subprocess.check_output([exe, "--no-gpu"]).decode()
        assert "checks ok" in out, out
