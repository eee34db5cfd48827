"""The linked-block decoder (LZ4_decompress_safe_continue over chains, liblz4's rolling-prefix mode) on the GPU against the reference
library's own stream decoder: the whole case set of tests/chain_common.py through the device call in one launch, again spread over
launches of 1, 33 and 2000 chains and of 40000 short chains (more chains than lane groups: the queue hands every group several), the
host call with chains of 1 to 70 blocks in one launch, the Python layer, the C++ mirror, the JNI shim, the opt-in frame reader and the
multi-device host path.  Guard bytes lie in front of every history, behind every region and between the chains; the damaged streams
are the kind the other decoder tests use."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from chain_common import CHAIN_STOPPED, Chain, Packed, RefChain, book1, case_set, chain_file, hand_chains, rng_for
from support import build_fake_jni, build_mirror, run_child
import streams_common as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rc(ref):
    return RefChain(ref)


@pytest.fixture(scope="module")
def cases(rc):
    """the chains and the reference's (out_len, chain_out_len, bytes) for each, computed once"""
    chains = case_set(rc, rng_for(21))
    return chains, [rc.decode(c) for c in chains]


def device_call(amd, pk, dev, with_optional=True):
    import torch
    d_src = torch.frombuffer(bytearray(pk.src), dtype=torch.uint8).to(dev)
    d_dst = torch.frombuffer(bytearray(pk.dst), dtype=torch.uint8).to(dev)
    i64 = lambda v: torch.tensor(np.asarray(v, dtype=np.int64), device=dev)
    i32 = lambda v: torch.tensor(np.asarray(v, dtype=np.int32), device=dev)
    out = torch.full((max(pk.n_blocks, 1),), -12345, dtype=torch.int32, device=dev)
    cout = torch.full((pk.n_chains,), -1, dtype=torch.int64, device=dev)
    stored = torch.tensor(np.asarray(pk.stored, dtype=np.uint8), device=dev) if with_optional else None
    prefix = i32(pk.prefix) if with_optional else None
    amd.DeviceBatch.decompress_safe_chain(d_src, i64(pk.src_off), i32(pk.src_len), i32(pk.dst_cap), i32(pk.chain_first), d_dst, i64(pk.chain_dst_off),
                                          i64(pk.chain_dst_cap), out, cout, prefix, stored)
    torch.cuda.synchronize()
    return d_dst.cpu().numpy().tobytes(), out.cpu().tolist()[:pk.n_blocks], cout.cpu().tolist()


def run_device(amd, chains, want, what):
    import torch
    pk = Packed(chains)
    dst, out, cout = device_call(amd, pk, torch.device("cuda", 0))
    bad = pk.check(dst, out, cout, want)
    assert not bad, (what, len(bad), bad[:5])


def test_chain_device_whole_set(amd, cases):
    """every chain of the set in ONE launch: chains of 1 to 70 blocks side by side in the wavefronts"""
    chains, want = cases
    assert len(chains) > 900 and sum(1 for w in want if CHAIN_STOPPED in w[0]) > 100
    run_device(amd, chains, want, "whole set")


@pytest.mark.parametrize("n_chains", (1, 33, 2000))
def test_chain_device_spread(amd, cases, n_chains):
    """the set again in launches of n_chains chains (2000: the set cycled)"""
    chains, want = cases
    if n_chains == 2000:
        idx = [i % len(chains) for i in range(2000)]
        run_device(amd, [chains[i] for i in idx], [want[i] for i in idx], "2000 chains")
        return
    for a in range(0, len(chains), n_chains):
        run_device(amd, chains[a:a + n_chains], want[a:a + n_chains], "launches of %d, from %d" % (n_chains, a))


def test_chain_device_more_chains_than_groups(amd, rc):
    """40000 short chains (the hand-built offset, end-of-block and straddle cases, cycled): more than the lane groups a launch can have,
    so every group draws several chains from the queue, of uneven length"""
    small = [c for c in hand_chains(rng_for(8)) if c.ccap + len(c.history) < 3000]
    w = [rc.decode(c) for c in small]
    assert len(small) > 300
    idx = [(i * 7) % len(small) for i in range(40000)]
    run_device(amd, [small[i] for i in idx], [w[i] for i in idx], "40000 chains")


def test_chain_device_without_optional_arrays(amd, cases):
    """stored == NULL and chain_prefix_len == NULL: the chains that need neither"""
    import torch
    chains, want = cases
    sel = [i for i, c in enumerate(chains) if not c.history and not any(st for _, st, _ in c.blocks)][:400]
    pk = Packed([chains[i] for i in sel])
    dst, out, cout = device_call(amd, pk, torch.device("cuda", 0), with_optional=False)
    bad = pk.check(dst, out, cout, [want[i] for i in sel])
    assert not bad, bad[:5]


def test_chain_host_call_and_python_layer(amd, cases):
    """the host call through LZ4HIPBatch.decompressSafeChain: the whole set in one call (chains of 1 to 70 blocks in one launch); only the
    decoded bytes come back -- every other byte of the caller's buffer is as it was"""
    chains, want = cases
    pk = Packed(chains)
    dst = bytearray(pk.dst)
    out, cout = amd.LZ4HIPBatch.decompressSafeChain(pk.src, pk.src_off, pk.src_len, pk.dst_cap, pk.chain_first, dst, pk.chain_dst_off, pk.chain_dst_cap,
                                                    pk.prefix, pk.stored)
    bad = pk.check(dst, out, cout, want)
    assert not bad, (len(bad), bad[:5])
    for c, (outs, done, _) in enumerate(want):   # behind the decoded bytes the region is untouched
        off = pk.chain_dst_off[c]
        assert dst[off + done:off + pk.chain_dst_cap[c]] == bytes([pk.fill]) * (pk.chain_dst_cap[c] - done), chains[c].name
    # numpy in, numpy out; no history, no stored blocks
    sel = [i for i, c in enumerate(chains) if not c.history and not any(st for _, st, _ in c.blocks)][:50]
    pk = Packed([chains[i] for i in sel])
    dst = bytearray(pk.dst)
    out, cout = amd.LZ4HIPBatch.decompressSafeChain(pk.src, np.array(pk.src_off, dtype=np.uint64), np.array(pk.src_len, dtype=np.int32),
                                                    np.array(pk.dst_cap, dtype=np.int32), np.array(pk.chain_first, dtype=np.uint32), dst,
                                                    np.array(pk.chain_dst_off, dtype=np.uint64), np.array(pk.chain_dst_cap, dtype=np.uint64))
    assert out.dtype == np.int32 and cout.dtype == np.uint64
    assert not pk.check(dst, out.tolist(), cout.tolist(), [want[i] for i in sel])


def test_chain_host_call_in_small_chunks(amd, cases, rc, monkeypatch):
    """the host call with 1 MiB chunks (LZ4HIP_HOST_CHUNK_MB=1, read per call): the set, cycled until its 16-byte-rounded streams pass
    2 MiB, is staged in three chunks or more through one buffer set, and a chain of seventeen stored 64 KiB blocks in the middle is
    larger than a chunk by itself (a chunk takes one chain at least).  The assertions of test_chain_host_call_and_python_layer"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    chains, want = cases
    rounded = lambda ch: sum((len(s) + 15) & ~15 for s, _, _ in ch.blocks)
    data = (book1() * 2)[:17 * 65536]
    big = Chain("17 stored x 65536", [(data[o:o + 65536], True, 65536) for o in range(0, len(data), 65536)])
    assert rounded(big) > 1 << 20
    sel, total = [], 0
    while total <= 2 << 20 or len(sel) < len(chains):
        sel.append(len(sel) % len(chains))
        total += rounded(chains[sel[-1]])
    assert total > 2 << 20
    use, w = [chains[i] for i in sel], [want[i] for i in sel]
    at = len(use) // 3
    use.insert(at, big)
    w.insert(at, rc.decode(big))
    assert w[at][1] == len(data)
    pk = Packed(use)
    dst = bytearray(pk.dst)
    out, cout = amd.LZ4HIPBatch.decompressSafeChain(pk.src, pk.src_off, pk.src_len, pk.dst_cap, pk.chain_first, dst, pk.chain_dst_off, pk.chain_dst_cap,
                                                    pk.prefix, pk.stored)
    bad = pk.check(dst, out, cout, w)
    assert not bad, (len(bad), bad[:5])
    for c, (outs, done, _) in enumerate(w):   # behind the decoded bytes the region is untouched
        off = pk.chain_dst_off[c]
        assert dst[off + done:off + pk.chain_dst_cap[c]] == bytes([pk.fill]) * (pk.chain_dst_cap[c] - done), use[c].name


def program_cases(cases):
    """a few chains of every kind for the C++ and JNI programs: reference-written, with history, with stored and empty blocks, hand-built,
    damaged (stopped early), tight capacities"""
    chains, want = cases
    picks, seen = [], set()
    for i, c in enumerate(chains):
        kind = c.name.split(" ")[0] + ("/h" if c.history else "") + ("/stopped" if CHAIN_STOPPED in want[i][0] else "")
        if kind not in seen and c.ccap < 400000 and c.blocks:
            seen.add(kind)
            picks.append(i)
    assert len(picks) >= 8
    return [(chains[i], want[i]) for i in picks]


def test_chain_cpp_mirror(cases, tmp_path):
    """tests/cpp/chain_mirror_test.cpp: LZ4HIPBatch::decompressSafeChain of host/lz4hip.hpp, two chains per call"""
    exe = build_mirror("chain_mirror_test", tmp_path)
    for ch, (outs, done, data) in program_cases(cases):
        (tmp_path / "c.bin").write_bytes(chain_file(ch))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path / "o.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (ch.name, p.returncode, p.stderr.decode()[-2000:])
        assert p.stdout.decode().split() == [str(o) for o in outs] + ["|", str(done)], ch.name
        assert (tmp_path / "o.bin").read_bytes() == data, ch.name


def test_chain_jni_program(cases, tmp_path):
    """tests/jni_stub/fake_jni_chain.c: the JNI shim's LZ4HIP_batchSafeChain over the fake JNIEnv"""
    exe = build_fake_jni("fake_jni_chain", tmp_path)
    for ch, (outs, done, data) in program_cases(cases):
        (tmp_path / "c.bin").write_bytes(chain_file(ch))
        p = subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0 and b"checks ok" in p.stdout, (ch.name, p.returncode, p.stderr.decode()[-2000:])
        assert (tmp_path / "chain.txt").read_text().split() == [str(o) for o in outs] + ["|", str(done)], ch.name
        assert (tmp_path / "chain.out").read_bytes() == data, ch.name


@pytest.fixture(scope="module")
def frame_data():
    b = book1()
    return b[:300000] + rng_for(9).randbytes(150000) + b[250000:420000]


def test_chain_frame_reader_with_the_engine(amd, rc, port, frame_data, tmp_path):
    """LZ4FrameInputStream(linkedBlocks=True) with HIPEngine, in Python and through host/lz4hip_streams.hpp: frames without block independence
    assembled from reference-written chains and, where the `lz4` command line is installed, written by it; batches of 1, 3 and 64 blocks
    (the carried 64 KB); the default reader refuses them"""
    import importlib
    import io
    from chain_common import linked_frame
    S = importlib.import_module("lz4-java_amd.streams")
    big = (book1() * 12)[:9000000]
    frames = [(linked_frame(rc, port.xxh32, frame_data, 4, block_checksum=True, content_checksum=True)[0], frame_data),
              (linked_frame(rc, port.xxh32, big, 7, content_size=True)[0], big)]
    if sc.LZ4_CLI is not None:
        frames += [(sc.cli(args, d), d) for args, d in ((["-1", "-B4", "-BD"], frame_data), (["-B4", "-BD", "-BX"], frame_data),
                                                        (["-B7", "-BD", "--content-size"], big))]
    exe = build_mirror("chain_mirror_test", tmp_path)
    for k, (frame, d) in enumerate(frames):
        assert frame[4] & 0x20 == 0
        for batch in (1, 3, 64):
            assert S.LZ4FrameInputStream(io.BytesIO(frame), batchBlocks=batch, linkedBlocks=True).read() == d, (k, batch)
        sc._expect(S, frame, "BLOCK_INDEPENDENCE", S.HIPEngine())
        (tmp_path / "f.lz4").write_bytes(frame)
        for batch in (1, 64):
            p = subprocess.run([exe, "--frame", str(tmp_path / "f.lz4"), str(tmp_path / "f.out"), str(batch)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               timeout=120)
            assert p.returncode == 0, (k, batch, p.stderr.decode()[-2000:])
            assert (tmp_path / "f.out").read_bytes() == d, (k, batch)


def test_chain_multidev_host_path_on_one_gpu():
    """lz4hip_init([0] * 2): the host call takes the multi-device branch (whole chains per listed device)"""
    assert "chain multidev ok D=2" in run_child("chain_multidev_child.py", "2", "repeat", timeout=600)


def test_chain_multidev_host_path_two_gpus():
    """two different devices: chains sharded at chain boundaries, each device decoding whole chains"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than two GPUs")
    assert "chain multidev ok D=2" in run_child("chain_multidev_child.py", "2", "distinct", timeout=600)
