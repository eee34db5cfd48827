"""The scratch layout of the HC chain compressor's layout kernel (staging::HcChainScratchLayout, lz4-java_amd/csrc/host_staging.h: where
its arrays lie and how many build items they have room for) without a device: tests/cpp/hcchain_scratch_test.cpp checks it against
restatements, built with the address and undefined-behaviour sanitizers and run as it is."""
import subprocess

from support import build_sanitized


def test_hcchain_scratch_program(tmp_path):
    exe = build_sanitized("hcchain_scratch_test", tmp_path)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout.decode().strip() == "ok", (p.returncode, p.stderr.decode()[-3000:])
