"""The stream decoder (LZ4_decompress_safe_continue in every mode of liblz4's LZ4_streamDecode_t) on the GPU against the reference
library's own stream decoder, one LZ4_streamDecode_t per stream, its four fields read back after every call: 64 streams of every
layout of tests/dstream_common.py cut into 2 to 6 calls with the state threaded through, 3000 streams x 3 calls on a ring (more
streams than lane groups: the queue, and the staging in more than one chunk), the hostile list, a round trip from CompressStreams into
a ring and into two alternating buffers, equality with the chain call where the blocks lie back to back, two host threads, the
multi-device host path, the C++ mirror and the JNI shim.  128 guard bytes of 0xEE lie around every window and behind every dictionary;
the whole destination is compared after every call, so a byte written anywhere but in a block's decoded range shows."""
import ctypes as C
import subprocess
import threading

import pytest

from dstream_common import (CHAIN_STOPPED, DICT, FILL, GUARD, Placed, RefStream, book1, check_set, hostile_set, layout_set, lib_decoder, make_stream,
                            padded_cuts, rng_for, run_placed, same_state, shared_dicts, stream_file)
from support import build_fake_jni, build_mirror, run_child

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rs(ref):
    return RefStream(ref)


@pytest.fixture(scope="module")
def decode(amd):
    return lib_decoder(amd.lib())


@pytest.mark.parametrize("layout", "abcdefg")
def test_dstream_layout(rs, decode, layout):
    """64 streams of one layout in 2 to 6 calls (layout c: its caller moves the history in front of every block, so a call per block
    and streams of at most 5 blocks)"""
    rng = rng_for(40 + ord(layout))
    data = book1()
    dicts = shared_dicts(data)
    streams = []
    for t in range(64):
        kw = dict(dictionary=dicts[(7, 4096, 70000)[t % 3]], lead=(t % 6 == 5)) if layout == "f" else {}
        if layout == "c":
            kw["n_blocks"] = rng.randrange(2, 5)
        streams.append(make_stream(rs, layout, rng, data, tag="#%d" % t, **kw))
    bad, calls = check_set(rs, streams, rng.randrange(2, 7), rng, decode, (layout,))
    assert not bad, (len(bad), bad[:5])
    assert 2 <= calls <= 6


def test_dstream_more_streams_than_groups(rs, decode, monkeypatch):
    """3000 streams x 3 calls of one 1 KiB block on a ring (layout d): more streams than a launch has lane groups, staged in chunks of
    1 MiB of compressed bytes (LZ4HIP_HOST_CHUNK_MB=1, read per call): three chunks or more per call"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    rng = rng_for(50)
    data = book1()
    streams = [rs.write("d1k #%d" % t, "d", 65535 + 2048, [data[o:o + 1024] for o in range(t * 64, t * 64 + 3072, 1024)],
                        lambda k, n, pos: pos if pos + n <= 65535 + 2048 else 0, True, zero_at_jump=False) for t in range(3000)]
    cuts = [[1, 2, 3]] * len(streams)
    wants = [rs.decode(s, c) for s, c in zip(streams, cuts)]
    bad = run_placed(streams, cuts, wants, decode, ("3000",))
    assert not bad, (len(bad), bad[:5])


def test_dstream_hostile(rs, decode):
    """a flipped byte per stream, offsets one past the reachable history with ext_len below and at least 65536, capacities one short,
    negative lengths -- results, states and every byte outside the failed blocks' slots"""
    rng = rng_for(51)
    streams = hostile_set(rs, rng, 8)
    bad, _ = check_set(rs, streams, 3, rng, decode, ("hostile",))
    assert not bad, (len(bad), bad[:5])
    stopped = sum(1 for s in streams for r in rs.decode(s, [len(s.blocks)]).out if r == CHAIN_STOPPED)
    assert stopped > 20


def test_dstream_equals_the_chain_call_where_blocks_lie_back_to_back(amd, rs, decode):
    """layout a without the 0-byte block: out_len and bytes are lz4hip_decompress_safe_chain_batch's"""
    rng = rng_for(52)
    data = book1()
    streams = [make_stream(rs, "a", rng, data, tag="#%d" % t, zero_at_jump=False) for t in range(64)]
    cuts = [[len(s.blocks)] for s in streams]
    p = Placed(streams, cuts)
    src, so, sl, first, do, dc, wo, wl, idx = p.call(0)
    rc, out, new = decode(p.state, src, so, sl, first, p.dst, do, dc, wo, wl)
    assert rc == 0
    chain_dst = bytearray(Placed(streams, cuts).dst)
    cout, clen = amd.LZ4HIPBatch.decompressSafeChain(src, so, sl, dc, first, chain_dst, wo, wl)
    assert list(cout) == out and bytes(chain_dst) == bytes(p.dst)
    assert [int(st[1]) for st in new] == [int(v) for v in clen]


def test_dstream_python_layer_and_two_threads(amd, rs):
    """DecodeStreams / LZ4HIPBatch.decompressSafeStream, from two host threads on disjoint stream sets at once"""
    def py_decode(ds):
        def f(state, src, so, sl, first, dst, do, dc, wo, wl):
            ids = list(range(len(state)))
            for c, st in enumerate(state):      # (what the caller's own LZ4_setStreamDecode calls left)
                if tuple(st) != ds.state([c])[0]:
                    ds.reset([c])
                    ds.set(c, st[0], st[1])
                    assert st[3] == 0
            out = ds.decompress(ids, src, so, sl, first, dst, do, dc, wo, wl)
            return 0, list(out), ds.state()
        return f
    res = [None, None]

    def work(k):
        rng = rng_for(60 + k)
        streams = [s for s in layout_set(rs, rng, 5) if not any(b.src_len < 0 or b.cap < 0 for b in s.blocks)]
        res[k] = check_set(rs, streams, 4, rng, py_decode(amd.DecodeStreams(len(streams))), ("thread %d" % k,))[0]
    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert res[0] == [] and res[1] == [], (res[0][:3] if res[0] else None, res[1][:3] if res[1] else None)


def test_dstream_round_trip_from_compress_streams(amd):
    """CompressStreams output, 64 streams x 4 calls of one block, decoded into a ring of 65535 + 2 x maxBlock (the compressor keeps
    its whole history) and into two alternating buffers (the compressor keeps one block of history)"""
    data = book1()
    n, bs = 64, 3000
    for layout, keep_blocks in (("d", 100), ("b", 1)):
        win_len = 65535 + 2 * bs if layout == "d" else 2 * bs
        with amd.CompressStreams(n) as cs:
            ds = amd.DecodeStreams(n)
            dst = bytearray([FILL]) * (n * (win_len + GUARD) + GUARD)
            win = [GUARD + t * (win_len + GUARD) for t in range(n)]
            pos = [0] * n
            for call in range(4):
                src, cso, pre, sl = bytearray(), [], [], []
                for t in range(n):
                    o = 1000 * t + call * bs
                    hist = min(call, keep_blocks) * bs
                    src += data[o - hist:o + bs] if hist else data[o:o + bs]
                    cso.append(len(src) - bs); pre.append(hist); sl.append(bs)
                comp = bytearray(n * (bs + 64))
                out, cons = cs.compress(list(range(n)), bytes(src), cso, sl, list(range(n + 1)), comp, [t * (bs + 64) for t in range(n)], [bs + 64] * n, pre)
                assert all(r > 0 for r in out) and list(cons) == [bs] * n
                do = []
                for t in range(n):
                    if layout == "b":
                        pos[t] = (call & 1) * bs
                    elif pos[t] + bs > win_len:
                        pos[t] = 0
                    do.append(win[t] + pos[t]); pos[t] += bs
                got = ds.decompress(list(range(n)), bytes(comp), [t * (bs + 64) for t in range(n)], list(out), list(range(n + 1)), dst, do, [bs] * n, win,
                                    [win_len] * n)
                assert list(got) == [bs] * n, (layout, call, list(got)[:8])
                for t in range(n):
                    o = 1000 * t + call * bs
                    assert dst[do[t]:do[t] + bs] == data[o:o + bs], (layout, call, t)
            for t in range(n):
                assert dst[win[t] - GUARD:win[t]] == bytes([FILL]) * GUARD


def program_streams(rs):
    """a few streams of every layout, hostile ones among them, for the C++ and JNI programs"""
    rng = rng_for(70)
    return [s for s in layout_set(rs, rng, 2) + hostile_set(rs, rng, 2) if not s.before and all(b.src_len >= 0 and b.cap >= 0 for b in s.blocks)][::3][:9]


def run_program(rs, exe, args, tmp_path):
    for s in program_streams(rs):
        n = len(s.blocks)
        cuts = [max(1, n // 2), n] if n > 1 else [n]
        w = rs.decode(s, cuts)
        (tmp_path / "s.bin").write_bytes(stream_file(s, cuts))
        p = subprocess.run([exe, str(tmp_path / "s.bin")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (s.name, p.returncode, p.stderr.decode()[-2000:])
        yield s, w, p.stdout.decode()


def check_program_output(s, w, text):
    """line 1: the results; line 2: the state behind the last call, ends relative to the window"""
    lines = text.splitlines()
    assert [int(v) for v in lines[0].split()] == w.out, (s.name, lines[0][:80], w.out[:8])
    pe, pl, ee, el = (int(v) for v in lines[1].split())
    D = len(s.dictionary) if s.dictionary else 0
    dict_end = 0 if s.lead else -(GUARD if D else 0)
    got = (DICT if (pl and D and not s.lead and pe == dict_end) else pe, pl, DICT if (el and D and not s.lead and ee == dict_end) else ee, el)
    assert same_state(got, w.states[-1]), (s.name, got, w.states[-1])


def test_dstream_cpp_mirror(rs, tmp_path):
    """tests/cpp/dstream_mirror_test.cpp: DecodeStreams of host/lz4hip.hpp, a stream in two calls"""
    exe = build_mirror("dstream_mirror_test", tmp_path)
    for s, w, text in run_program(rs, exe, [], tmp_path):
        check_program_output(s, w, text)


def test_dstream_jni_program(rs, tmp_path):
    """tests/jni_stub/fake_jni_dstream.c: the JNI shim's LZ4HIP_batchSafeStream over the fake JNIEnv"""
    exe = build_fake_jni("fake_jni_dstream", tmp_path)
    for s, w, text in run_program(rs, exe, [], tmp_path):
        assert "checks ok" in text, s.name
        check_program_output(s, w, text)


def test_dstream_multidev_host_path_on_one_gpu():
    """lz4hip_init([0] * 2): the host call takes the multi-device branch (whole streams per listed device)"""
    assert "dstream multidev ok D=2" in run_child("dstream_multidev_child.py", "2", "repeat", timeout=600)


def test_dstream_multidev_host_path_two_gpus():
    """two different devices: streams sharded at stream boundaries, each device decoding whole streams"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than two GPUs")
    assert "dstream multidev ok D=2" in run_child("dstream_multidev_child.py", "2", "distinct", timeout=600)
