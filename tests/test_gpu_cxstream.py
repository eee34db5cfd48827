"""lz4hip_compress_fast_stream_ext_batch on the GPU -- resident compress streams whose sources land anywhere -- against ONE LZ4_stream_t
of the reference library per stream (tests/cxstream_common.py): 64 streams of every layout, 3000 streams on two alternating buffers
staged in chunks, the hand-built list, stops, resets and lz4hip_cstreams_consumed, the two entry points alternating on one set, a fresh
stream with a dictionary elsewhere against lz4hip_compress_fast_dict_batch, two host threads on two sets, a set divided over device
entries, the C++ and fake-JNI programs.  Where the slots of a decoder on the same layout stay clear of the history it can reach
(contiguous, two buffers, the save area, the ring of 65535 + 2 x maxBlock) the output is also decoded with DecodeStreams on that layout
and compared with the input.  Guard bytes lie around every destination slot.

A call is a snapshot of the producer's memory, so a stream whose producer writes over its window takes a call per stretch of blocks
that do not land on one another's reach; every call carries all the streams that still have blocks."""
import ctypes as C
import random
import subprocess
import threading

import numpy as np
import pytest

from cchain_common import CHAIN_STOPPED, bound
from cxstream_common import (GUARD, LAYOUTS, DevX, PackedX, RefX, XBlock, XStream, book1, capacity_case, drive_x, hand_built, jump_share, make_xstream)
from dstream_common import RefStream, cut_pieces
from support import build_fake_jni, build_mirror, run_child
from test_cxstream_abi import stream_file

pytestmark = pytest.mark.gpu
DECODABLE = ("contig", "two4096", "save", "ring73727")
u64, i32, u32, u8 = C.c_uint64, C.c_int32, C.c_uint32, C.c_uint8


@pytest.fixture(scope="module")
def rs(ref):
    return RefStream(ref)


def decode_back(amd, streams, made, kept):
    """the engine's output through DecodeStreams on the same layout: every stream has an arena like the encoder's; behind every call
    the bytes of the call's blocks are the input's"""
    sizes = [GUARD + len(xs.dictionary or b"") + GUARD + xs.win_len + GUARD for xs in streams]
    base = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    win = [b + GUARD + len(xs.dictionary or b"") + GUARD for b, xs in zip(base, streams)]
    dst = bytearray(b"\xEE" * sum(sizes))
    ds = amd.DecodeStreams(len(streams))
    nth = [0] * len(streams)
    for rounds, now, pk, out, comp in kept:
        do, dc, wo, wl = [], [], [], []
        for t, i in enumerate(now):
            xs, c = streams[i], made[i][nth[i]]
            if xs.save_area and c.k0:      # the decoder's caller moves the last 64 KB in front of the block area, as the encoder's did
                keep = c.hist_len
                end = win[i] + xs.save_area + len(xs.blocks[c.k0 - 1].data)
                dst[win[i] + xs.save_area - keep:win[i] + xs.save_area] = bytes(dst[end - keep:end])
                ds.reset([i]); ds.set(i, win[i] + xs.save_area, keep)
            for b in c.blocks:
                do.append(win[i] + b.off); dc.append(len(b.data))
            wo.append(win[i]); wl.append(xs.win_len)
        got = ds.decompress(list(now), bytes(comp), pk.dst_off, out, pk.first, dst, do, dc, wo, wl)
        assert list(got) == dc, (rounds, list(got)[:8], dc[:8])
        k = 0
        for t, i in enumerate(now):
            for b in made[i][nth[i]].blocks:
                assert dst[do[k]:do[k] + dc[k]] == b.data, (streams[i].name, rounds)
                k += 1
            nth[i] += 1


@pytest.mark.parametrize("layout", LAYOUTS)
def test_layout(amd, rs, layout):
    """64 streams of one layout against the reference, every stream in every call"""
    rng = random.Random(200 + LAYOUTS.index(layout))
    data = book1()
    streams = [make_xstream(layout, rng, data, "#%d" % t) for t in range(64)]
    eng = DevX(amd, 70)
    ids = sorted(rng.sample(range(70), 64))
    kept = []
    bad, made, rounds = drive_x(eng, rs, streams, rng, mode="random", ids=ids, absent=0.0, keep=kept)
    assert not bad, (len(bad), bad[:5])
    assert rounds >= 2
    cons, stop = eng.consumed()
    assert [cons[i] for i in ids] == [sum(len(b.data) for b in xs.blocks) for xs in streams] and not any(stop)
    if layout in DECODABLE:
        decode_back(amd, streams, made, kept)
    eng.close()


def test_more_streams_than_wavefronts(amd, rs, monkeypatch):
    """3000 streams x 3 calls of one block of at most 1 KiB on two alternating buffers: more streams than a launch has wavefronts
    (5 x 256), staged in chunks of 1 MiB (LZ4HIP_HOST_CHUNK_MB=1, read per call)"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    rng = random.Random(220)
    data = book1()
    streams = []
    for t in range(3000):
        o = 97 * t
        sizes = [rng.randrange(1, 1025) for _ in range(3)]
        blocks = [XBlock((k & 1) * 1024, data[o + 700 * k:o + 700 * k + n]) for k, n in enumerate(sizes)]
        streams.append(XStream("3000 #%d" % t, "two1024", 2048, blocks))
    eng = DevX(amd, 3000)
    bad, made, rounds = drive_x(eng, rs, streams, rng, mode="every", absent=0.0)
    assert not bad and rounds == 3, (rounds, len(bad), bad[:5])
    d, t = jump_share(rs, streams[:200], made[:200])     # (the first of three blocks cannot differ, and a block of a few hundred bytes
    assert d > 0, (d, t)                                  # finds little in the one before it: the history elsewhere matters in some)
    eng.close()


def test_hand_built_stops_resets_and_consumed(amd, rs):
    """the hand-built list; a capacity one short at a jump stops the stream -- LZ4HIP_CHAIN_STOPPED in later calls, nothing consumed,
    reported by lz4hip_cstreams_consumed -- until it is reset; the streams beside it are untouched"""
    data = book1()
    rng = random.Random(230)
    streams = hand_built(rng, data)
    eng = DevX(amd, len(streams))
    bad, made, _ = drive_x(eng, rs, streams, rng, mode="every", absent=0.0)
    assert not bad, (len(bad), bad[:5])
    eng.reset()
    bad, made, _ = drive_x(eng, rs, streams, rng, mode="none", absent=0.3)
    assert not bad, (len(bad), bad[:5])
    eng.close()
    xs = capacity_case(rs, data)
    other = XStream("beside", "hand", 8192, [XBlock(b.off, b.data) for b in xs.blocks])
    eng = DevX(amd, 3)
    bad, made, _ = drive_x(eng, rs, [xs, other], rng, mode="every", ids=[0, 2], absent=0.0)
    assert not bad, bad
    assert [r for c in made[0] for r in c.outs][1:] == [0, CHAIN_STOPPED, CHAIN_STOPPED] and all(r > 0 for c in made[1] for r in c.outs)
    cons, stop = eng.consumed()
    assert cons == [len(xs.blocks[0].data), 0, sum(len(b.data) for b in other.blocks)] and stop == [1, 0, 0]
    eng.reset([0])
    assert eng.consumed() == ([0, 0, cons[2]], [0, 0, 0])
    again = XStream("after the reset", "hand", 8192, [XBlock(b.off, b.data) for b in xs.blocks])
    bad, made, _ = drive_x(eng, rs, [again], rng, mode="none", ids=[0], absent=0.0)
    assert not bad and all(r > 0 for c in made[0] for r in c.outs)
    # the id errors need a live set
    c = RefX(rs, other)
    pk = PackedX([c.next_call(1)], rng)
    c.close()
    eng.call([3], pk, expect=-3)
    eng.close()


def test_entry_points_alternate_on_one_set(amd, rs):
    """lz4hip_compress_fast_stream_batch and lz4hip_compress_fast_stream_ext_batch take turns on the streams of one set: the bytes are
    ONE LZ4_stream_t's, whichever entry takes a call"""
    data = book1()
    rng = random.Random(240)
    n = 24
    eng = DevX(amd, n)
    streams, refs = [], []
    for t in range(n):
        pieces = cut_pieces(data, rng, 12, 0, 3000)
        offs, pos = [], 0
        for k, p in enumerate(pieces):     # contiguous, but every fourth block jumps to a place of its own further up
            if k and k % 4 == 0:
                pos += 5000
            offs.append(pos); pos += len(p)
        streams.append(XStream("alternating %d" % t, "contig", pos + 16, [XBlock(o, p) for o, p in zip(offs, pieces)]))
        refs.append(RefX(rs, streams[-1]))
    for k in range(12):
        calls = [r.next_call(k + 1) for r in refs]
        if k % 4 == 0 or k % 4 == 2:
            pk = PackedX(calls, rng)
            dst, out, cons = eng.call(list(range(n)), pk)
            assert not pk.check([s.name for s in streams], dst, out, cons), k
        else:   # the existing call: every stream's history lies directly in front of its source, in the arena as it stands
            src, cso, pre, sl, do, dc = bytearray(), [], [], [], [], []
            for t, c in enumerate(calls):
                s = refs[t].win_off + streams[t].blocks[k].off
                assert c.hist_end in (s, 0)
                cso.append(len(src) + s); pre.append(c.hist_len); sl.append(len(streams[t].blocks[k].data))
                do.append(t * 3200); dc.append(bound(sl[-1]))
                src += c.arena
            dst = bytearray(n * 3200)
            out, cons = amd.LZ4HIPBatch.compressFastStream(eng_set(amd, eng), list(range(n)), bytes(src), cso, sl, list(range(n + 1)), dst, do, dc, pre)
            for t, c in enumerate(calls):
                assert int(out[t]) == c.outs[0] and bytes(dst[do[t]:do[t] + c.outs[0]]) == c.by[0], (k, t)
    for r in refs:
        r.close()
    eng.close()


def eng_set(amd, eng):
    """the DevX engine's handle as the Python layer's set object"""
    class Set:
        def __len__(self):
            return eng.n

        def _handle(self):
            return eng.h
    return Set()


def test_fresh_stream_with_a_dictionary_elsewhere_is_the_dictionary_call(amd, rs):
    """a fresh stream whose first block does not follow its history equals lz4hip_compress_fast_dict_batch's block, byte for byte"""
    data = book1()
    rng = random.Random(250)
    for size in (7, 4096, 70000):
        d = data[100000:100000 + size]
        blocks = [data[o:o + n] for o, n in ((100000 + size - 50, 3000), (5000, 12), (100100, 4096), (300000, 0), (100000 + max(size - 70000, 0), 20000))]
        streams = [XStream("dict %d #%d" % (size, t), "contig", len(b) + 16, [XBlock(0, b)], dictionary=d, side=("front", "back")[t & 1]) for t, b in enumerate(blocks)]
        eng = DevX(amd, len(streams))
        kept = []
        bad, made, _ = drive_x(eng, rs, streams, rng, mode="none", absent=0.0, keep=kept)
        assert not bad, (size, bad[:3])
        eng.close()
        src = b"".join(blocks)
        so = np.concatenate([[0], np.cumsum([len(b) for b in blocks])[:-1]]).tolist()
        caps = [bound(len(b)) for b in blocks]
        do = np.concatenate([[0], np.cumsum(caps)[:-1]]).tolist()
        dst = bytearray(sum(caps))
        with amd.LZ4Dictionary(d) as handle:
            out = amd.LZ4HIPBatch.compressDict(src, so, [len(b) for b in blocks], dst, do, caps, handle)
        for t in range(len(blocks)):
            assert int(out[t]) == made[t][0].outs[0] and bytes(dst[do[t]:do[t] + int(out[t])]) == made[t][0].by[0], (size, t)


def test_two_host_threads_on_two_sets(amd, ref):
    """two sets, each driven from a thread of its own at the same time"""
    res = [None, None]

    def work(k):
        rng = random.Random(260 + k)
        data = book1()
        streams = [make_xstream(("two4096", "ring8192", "dict4096", "ring3000")[t % 4], rng, data, "thread %d #%d" % (k, t), n_blocks=8) for t in range(24)]
        eng = DevX(amd, len(streams))
        res[k] = drive_x(eng, RefStream(ref), streams, rng, mode="random", absent=0.2)[0]
        eng.close()
    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert res[0] == [] and res[1] == [], (res[0][:3] if res[0] else None, res[1][:3] if res[1] else None)


def program_streams(rs):
    rng = random.Random(270)
    data = book1()
    out = [make_xstream(lay, rng, data, "program", n_blocks=nb) for lay, nb in (("two4096", 7), ("ring8192", 14), ("ring3000", 9), ("contig", 5), ("two16", 11))]
    return out + hand_built(rng, data)[38:42]


def run_program(rs, exe, tmp_path, txt, outf):
    for xs in program_streams(rs):
        r = RefX(rs, xs)
        calls = []
        while r.k < len(xs.blocks):
            calls.append(r.next_call(min(len(xs.blocks), r.k + 3)))
        r.close()
        rel = lambda c: (c.k1, c.hist_end - c.blk_base if c.hist_len else 0, c.hist_len)
        (tmp_path / "s.bin").write_bytes(stream_file(xs.win_len, [rel(c) for c in calls], [(b.off, b.data, b.cap) for b in xs.blocks]))
        p = subprocess.run([exe, str(tmp_path / "s.bin"), str(tmp_path / outf)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (xs.name, p.returncode, p.stderr.decode()[-2000:])
        yield xs, calls, p.stdout.decode()


def test_cpp_mirror(rs, tmp_path):
    """tests/cpp/cxstream_mirror_test.cpp: CompressStreams::compressAt of host/lz4hip.hpp, call after call"""
    exe = build_mirror("cxstream_mirror_test", tmp_path)
    for xs, calls, text in run_program(rs, exe, tmp_path, None, "o.bin"):
        assert [int(v) for v in text.split()] == [r for c in calls for r in c.outs], xs.name
        assert (tmp_path / "o.bin").read_bytes() == b"".join(x for c in calls for x in c.by), xs.name


def test_jni_program(rs, tmp_path):
    """tests/jni_stub/fake_jni_cxstream.c: the JNI shim's LZ4HIP_batchFastStreamAt over the fake JNIEnv"""
    exe = build_fake_jni("fake_jni_cxstream", tmp_path)
    (tmp_path / "out").mkdir()
    for xs, calls, text in run_program(rs, exe, tmp_path, None, "out"):
        assert "checks ok" in text, xs.name
        assert [int(v) for v in (tmp_path / "out" / "cxstream.txt").read_text().split()] == [r for c in calls for r in c.outs], xs.name
        assert (tmp_path / "out" / "cxstream.out").read_bytes() == b"".join(x for c in calls for x in c.by), xs.name


def test_multidev_host_path_on_one_gpu():
    """lz4hip_init([0] * 3): the set has three parts and every call is sharded at their boundaries"""
    assert "cxstream multidev ok" in run_child("cxstream_multidev_child.py", 3, timeout=120)


def test_multidev_host_path_two_gpus():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than two GPUs")
    assert "cxstream multidev ok" in run_child("cxstream_multidev_child.py", 0, timeout=120)
