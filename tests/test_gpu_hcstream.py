"""lz4hip_compress_hc_stream_batch on the GPU: HC streams whose sources land anywhere, every stream against the reference library's ONE
LZ4_streamHC_t on a real arena (tests/hcstream_common.py) -- bytes, return values and the written-back state.  64 streams per layout in
2 .. 6 calls, more streams than a launch has wavefronts, the hand-built list, equality with the chain call on streams that never jump
and with the dictionary call on a fresh stream, the way back through the stream decoder, two host threads, the multi-device branch."""
import random
import subprocess
import threading

import pytest

from cchain_common import book1, bound
from hcstream_common import (MAXB, Fleet, RefHCStream, capacity_scripts, compare, cut_into_calls, drive, hand_scripts, lay_contiguous, lay_dict_elsewhere,
                             lay_ring, lay_save_area, lay_two_buffers, make, read_results, script_file, sizes_of)
from support import build_fake_jni, build_mirror, run_child

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rr(ref):
    return RefHCStream(ref)


LAYOUTS = ("contiguous", "two", "adjacent", "ring", "save", "dict")


@pytest.mark.parametrize("level", (1, 9, 12))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layout(amd, rr, layout, level):
    """64 streams of one layout (16 blocks of at most 1 KiB) against the reference, cut into 2 .. 6 calls where the snapshot rule and the
    state edits leave the choice"""
    rng = random.Random(300 + LAYOUTS.index(layout))
    data = book1()
    scripts = [make(layout, data[rng.randrange(0, 600000):], rng, "#%d" % i) for i in range(64)]
    left_out = []
    bad, fleet = drive(amd, rr, scripts, level, rng, "few", left_out)
    assert not bad, (len(bad), bad[:5])
    assert not left_out, left_out[:5]          # (these streams are younger than 64 KB: the stated exception of levels 10..12 does not apply)
    # (a double buffer, a ring that wraps and a save area force more calls: the next block lands on what an earlier one reads, and
    # LZ4_saveDictHC stands between two calls)
    assert 2 <= fleet.rounds <= 6 if layout in ("contiguous", "dict") else fleet.rounds >= 2, fleet.rounds


def test_large_ring_and_long_prefix(amd, rr):
    """the cases that need 64 KB of history: a ring of 65535 + 2 x 4096 bytes that wraps, prefixes of 65534 .. 65536 bytes with an
    external piece present, save areas that keep 64 KB; levels 9 and 10.  Levels 10..12 name and count what they leave out"""
    rng = random.Random(320)
    data = book1()
    big = data[20000:20000 + 65535 + 8 * MAXB]
    scripts = [lay_ring("big", big, sizes_of(rng, len(big)), 65535 + 2 * MAXB)] + [s for s in hand_scripts(rng) if "with an external piece" in s.name] + \
        [lay_save_area("big", data[:24 * MAXB], sizes_of(rng, 24 * MAXB), k) for k in (65536, 70000)]
    for level in (9, 10):
        left_out = []
        bad, _ = drive(amd, rr, scripts, level, rng, left_out=left_out)
        assert not bad, (level, len(bad), bad[:5])
        print("level %d, left out: %d blocks" % (level, len(left_out)), left_out[:3])
        assert not left_out, left_out[:5]   # (if a block ever differs under the stated exception: pin the exact named set here)


def test_more_streams_than_wavefronts(amd, rr, monkeypatch):
    """3000 streams x 3 calls of one block of at most 512 bytes on two adjacent buffers (a double buffer allows one block per call: the
    next block lands on what this one reads as its dictionary), staged in chunks of 1 MiB"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    rng = random.Random(330)
    data = book1()
    scripts = []
    for i in range(3000):
        d = data[rng.randrange(0, 700000):][:3 * 512]
        scripts.append(lay_two_buffers("#%d" % i, d, [512 if rng.random() < 0.5 else rng.randrange(14, 513) for _ in range(3)], 0, 512))
    fleet = Fleet(amd, scripts, 9)
    got = fleet.run([[[0], [1], [2]] for _ in scripts])
    bad = []
    for sc, g in zip(scripts, got):
        compare(sc, rr.run(sc, 9), g, 9, bad)
    assert not bad, (len(bad), bad[:5])
    assert fleet.rounds == 3


@pytest.mark.parametrize("level", (1, 9, 10, 12))
def test_hand_built(amd, rr, level):
    """the hand-built list and its capacity variants (the bound, one less, the result, one less, 0 and negative values and lengths in
    mid-stream: a block that returns 0 does not end its stream), a call per block and as few calls as the snapshot rule allows"""
    rng = random.Random(340)
    hand = hand_scripts(rng)
    scripts = hand + capacity_scripts(rr, hand[::7])
    for how in ("each", "one"):
        left_out = []
        bad, _ = drive(amd, rr, scripts, level, rng, how, left_out)
        assert not bad, (how, len(bad), bad[:5])
        assert not left_out, left_out[:5]


def test_never_jumping_streams_are_the_chain_call(amd):
    """streams that never jump, cut into calls, equal lz4hip_compress_hc_chain_batch over the same blocks in one call"""
    rng = random.Random(350)
    data = book1()
    scripts = [lay_contiguous("#%d" % i, data[rng.randrange(0, 500000):][:12 * 1024], sizes_of(rng, 12 * 1024, 1024)) for i in range(32)]
    for level in (9, 12):
        fleet = Fleet(amd, scripts, level)
        got = fleet.run([cut_into_calls(sc, "random", rng) for sc in scripts])
        src = b"".join(b"".join(o.data for o in sc.ops) for sc in scripts)
        lens = [o.n for sc in scripts for o in sc.ops]
        caps = [o.cap for sc in scripts for o in sc.ops]
        first, cso, p = [0], [], 0
        for sc in scripts:
            cso.append(p); p += sum(o.n for o in sc.ops); first.append(first[-1] + len(sc.ops))
        doff = [sum(caps[:i]) for i in range(len(caps))]
        dst = bytearray(sum(caps))
        out = amd.LZ4HIPBatch.compressHCChain(src, cso, lens, first, dst, doff, caps, None, level)
        k = 0
        for g in got:
            for r in g:
                assert (r[1], r[2]) == (out[k], bytes(dst[doff[k]:doff[k] + out[k]])), (level, k)
                k += 1


def test_fresh_stream_with_a_dictionary_elsewhere_is_the_dictionary_call(amd):
    """a fresh stream plus LZ4_loadDictHC of a dictionary elsewhere plus one block equals lz4hip_compress_hc_dict_batch's block"""
    rng = random.Random(360)
    data = book1()
    dic = data[400000:400000 + 5000]
    blocks = [data[rng.randrange(0, 300000):][:rng.randrange(0, 3000)] for _ in range(24)]
    scripts = [lay_dict_elsewhere("#%d" % i, dic, b, [len(b)]) for i, b in enumerate(blocks)]
    for level in (9, 11):
        fleet = Fleet(amd, scripts, level)
        got = fleet.run([cut_into_calls(sc, "one") for sc in scripts])
        with amd.LZ4Dictionary(dic) as d:
            src = b"".join(blocks)
            so = [sum(len(x) for x in blocks[:i]) for i in range(len(blocks))]
            caps = [bound(len(b)) for b in blocks]
            doff = [sum(caps[:i]) for i in range(len(caps))]
            dst = bytearray(sum(caps))
            out = amd.LZ4HIPBatch.compressHCDict(src, so, [len(b) for b in blocks], dst, doff, caps, d, level)
        for k, g in enumerate(got):
            assert (g[1][1], g[1][2]) == (out[k], bytes(dst[doff[k]:doff[k] + out[k]])), (level, k)


@pytest.mark.parametrize("layout", ("contiguous", "two", "adjacent", "ring", "save", "dict", "bigring"))
def test_back_through_the_stream_decoder(amd, layout):
    """what the stream compressor wrote decodes, through DecodeStreams into the same layout, to what was compressed (a call per block:
    the decoder's ring rule): every layout, the save area (the decoder's caller copies the kept bytes and says LZ4_setStreamDecode, as
    the compressor's caller says LZ4_saveDictHC), the dictionary elsewhere and the ring of 65535 + 2 x 4096 bytes included"""
    rng = random.Random(370)
    data = book1()
    if layout == "bigring":
        big = data[30000:30000 + 65535 + 8 * MAXB]
        scripts = [lay_ring("big", big, sizes_of(rng, len(big), tiny=False), 65535 + 2 * MAXB)]
    else:
        scripts = [make(layout, data[rng.randrange(0, 600000):], rng, "#%d" % i, n_blocks=8) for i in range(8)]
    fleet = Fleet(amd, scripts, 9)
    got = fleet.run([cut_into_calls(sc, "random", rng) for sc in scripts])
    back = bytearray(len(fleet.src))
    for sc, b in zip(scripts, fleet.base):
        for off, by in sc.init:
            back[b + off:b + off + len(by)] = by
    ds = amd.DecodeStreams(len(scripts))
    n_blocks = 0
    for step in range(max(len(sc.ops) for sc in scripts)):
        ids, comp, so, sl, first, doff, dcap, wo, wl = [], b"", [], [], [0], [], [], [], []
        for s, sc in enumerate(scripts):
            if step >= len(sc.ops):
                continue
            o, r, b = sc.ops[step], got[s][step], fleet.base[s]
            if o.kind == "L":
                ds.set(s, b + o.off, min(o.n, 65536))
            elif o.kind == "S":
                end, kept = ds.state([s])[0][0], r[1]
                back[b + o.off:b + o.off + kept] = bytes(back[end - kept:end])
                ds.set(s, b + o.off + kept, kept)
            else:
                assert r[1] > 0
                ids.append(s); so.append(len(comp)); sl.append(r[1]); comp += r[2]; first.append(len(so))
                doff.append(b + o.off); dcap.append(o.n); wo.append(b); wl.append(sc.arena)
        if not ids:
            continue
        out = ds.decompress(ids, comp, so, sl, first, back, doff, dcap, wo, wl)
        assert list(out) == dcap, (layout, step)
        for s, sc in enumerate(scripts):
            if step < len(sc.ops) and sc.ops[step].kind == "B":
                o = sc.ops[step]
                assert bytes(back[fleet.base[s] + o.off:fleet.base[s] + o.off + o.n]) == o.data, (layout, s, step)
                n_blocks += 1
    assert n_blocks == sum(len(sc.blocks()) for sc in scripts)


def test_two_host_threads(amd, rr):
    """two sets of streams, each driven from a thread of its own at the same time"""
    data = book1()
    res = [None, None]

    def work(k):
        rng = random.Random(380 + k)
        scripts = [make(("two", "ring")[k], data[rng.randrange(0, 600000):], rng, "#%d" % i) for i in range(24)]
        for sc in scripts:
            rr.run(sc, 9)
        res[k] = (scripts, rng)
    for k in range(2):
        work(k)             # (the reference's results first, on this thread: the memo is not shared work)
    out = [None, None]

    def go(k):
        scripts, rng = res[k]
        out[k] = drive(amd, rr, scripts, 9, rng)[0]
    th = [threading.Thread(target=go, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert out[0] == [] and out[1] == [], out


def test_cpp_mirror(rr, tmp_path):
    """tests/cpp/hcstream_mirror_test.cpp: CompressStreamsHC of host/lz4hip.hpp, a call per block, with loadDict and saveDict"""
    exe = build_mirror("hcstream_mirror_test", tmp_path, werror=True)
    rng = random.Random(385)
    data = book1()
    scripts = [make(lay, data[50000:], rng, "cpp", maxb=2048, n_blocks=6) for lay in ("adjacent", "ring", "save", "dict")] + hand_scripts(rng)[::11]
    bad = []
    for k, sc in enumerate(scripts):
        level = (9, 12, 3)[k % 3]
        fin, fout = tmp_path / ("s%d.bin" % k), tmp_path / ("o%d.bin" % k)
        fin.write_bytes(script_file(sc, level))
        subprocess.check_call([exe, str(fin), str(fout)])
        compare(sc, rr.run(sc, level), read_results(sc, fout.read_bytes()), level, bad)
    assert not bad, bad[:5]


def test_jni_program(rr, tmp_path):
    """tests/jni_stub/fake_jni_hcstream.c: the JNI shim's LZ4HIP_batchHCStream over the fake JNIEnv, a call per block"""
    exe = build_fake_jni("fake_jni_hcstream", tmp_path)
    rng = random.Random(386)
    data = book1()
    scripts = [make(lay, data[90000:], rng, "jni", maxb=2048, n_blocks=6) for lay in ("two", "ring", "save", "dict")] + hand_scripts(rng)[3::11]
    bad = []
    for k, sc in enumerate(scripts):
        level = (9, 10, 4)[k % 3]
        fin, fout = tmp_path / ("s%d.bin" % k), tmp_path / ("o%d.bin" % k)
        fin.write_bytes(script_file(sc, level))
        assert "checks ok" in subprocess.check_output([exe, str(fin), str(fout)]).decode()
        compare(sc, rr.run(sc, level), read_results(sc, fout.read_bytes()), level, bad)
    assert not bad, bad[:5]


def test_multidev_host_path_on_one_gpu():
    """lz4hip_init([0] * 3): every call is sharded over three engine devices at stream boundaries"""
    assert "hcstream multidev ok" in run_child("hcstream_multidev_child.py", 3, timeout=120)


def test_multidev_host_path_two_gpus():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than two GPUs")
    assert "hcstream multidev ok" in run_child("hcstream_multidev_child.py", 0, timeout=120)
