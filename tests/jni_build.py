"""Builds one of the fake-JNI programs of tests/jni_stub/ (the JNI shim over the fake JNIEnv of fake_env.h, linked with liblz4hip.so)
for the tests that run it."""
import os
import subprocess

from conftest import ROOT


def build_fake_jni(name, out_dir):
    """tests/jni_stub/<name>.c + the shim (malloc / free counted) -> the executable <out_dir>/<name>; returns its path"""
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "jni_stub", "build.sh"), name, str(out_dir)])
    return os.path.join(str(out_dir), name)
