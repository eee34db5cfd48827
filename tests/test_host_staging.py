"""The arithmetic of the host-pointer staging (lz4-java_amd/csrc/host_staging.h: metadata layouts, chunk cut, run plan, chain-shape
check) without a device: tests/cpp/host_staging_test.cpp checks each piece against a naive restatement, built with the address and
undefined-behaviour sanitizers and run as it is."""
import subprocess

from support import build_sanitized


def test_host_staging_program(tmp_path):
    exe = build_sanitized("host_staging_test", tmp_path)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout.decode().strip() == "ok", (p.returncode, p.stderr.decode()[-3000:])
