"""The in-order stream decoder (lz4hip_decompress_safe_stream_inorder_batch) on the GPU: streams whose slots overlap the history they can
reach -- liblz4's minimal rings, rings in step with the writer's, the grid of hand-built two-block streams -- against the reference
library's LZ4_decompress_safe_continue (one LZ4_streamDecode_t per stream) and, on the grid, against the plain definition; the exact
layouts a .. f and the hostile list with every block sent through the in-order tier; equality with the existing entry point; a round
trip from CompressStreams.compressAt on a ring in step with the writer; two host threads; the C++ mirror and the fake-JNI program; the
multi-device host path.  128 guard bytes of 0xEE lie around every window; the whole destination is compared after every call -- with
the replay of the reference's decoded bytes block by block in order -- so a byte stored past a block's result shows."""
import subprocess
import threading

import pytest

from dstream_common import (FILL, GUARD, Placed, RefStream, book1, check_set, hostile_set, layout_set, lib_decoder, padded_cuts, rng_for, same_state,
                            stream_file)
from dstream_inorder_common import GRID_WIN, behind_grid, grid, grid_expected, inorder_decoder, layout_streams, ring_size
from support import build_fake_jni, build_mirror, run_child
from test_dstream_inorder_plain import SEED_GRID

pytestmark = pytest.mark.gpu

# 24 streams per new layout: max_block 64 and 1024 keep the minimal rings' uploads small, 4096 for one stream set only
KINDS = [("m", "fit", 64, False), ("m", "fit", 1024, True), ("m", "max", 64, True), ("m", "max", 1024, False), ("m", "fit", 4096, True),
         ("g",), ("s", 8192, 1, 1500), ("s", 4096, 1, 1000), ("s", 1024, 1, 300), ("s", 70000, 1, 4096)]


@pytest.fixture(scope="module")
def rs(ref):
    return RefStream(ref)


@pytest.fixture(scope="module")
def decode(amd):
    return inorder_decoder(amd.lib())


@pytest.fixture()
def every_block(amd):
    """the knob at 1 for one test, 0 again behind it"""
    amd.set_option("dstream_inorder", 1)
    yield
    amd.set_option("dstream_inorder", 0)


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: "-".join(str(v) for v in k))
def test_inorder_layout(rs, decode, kind):
    """24 streams of one overlap layout in 2 to 6 calls, the state threaded through: results, states, and every byte of the destination"""
    rng = rng_for(90 + KINDS.index(kind))
    streams = layout_streams(rs, rng, kind, 24)
    bad, calls = check_set(rs, streams, rng.randrange(2, 7), rng, decode, kind)
    assert not bad, (len(bad), bad[:5])
    assert 2 <= calls <= 6


def test_inorder_grid_in_one_call(decode):
    """the grid as ONE call of many two-block streams -- the source 1 .. 200 bytes ahead of its destination in all three tails, and
    1 .. 100 bytes BEHIND it with a longer match: every window is the plain definition's, byte for byte, and the guards stand"""
    cases = grid(rng_for(SEED_GRID)) + behind_grid(rng_for(SEED_GRID + 1))
    streams = [c.stream for c in cases]
    p = Placed(streams, [[2]] * len(streams))
    src, so, sl, first, do, dc, wo, wl, idx = p.call(0)
    rc, out, new = decode(p.state, src, so, sl, first, p.dst, do, dc, wo, wl)
    assert rc == 0
    bad = []
    model = bytearray(p.model)
    for i, c in enumerate(cases):
        want, rr = grid_expected(c)
        if out[2 * i:2 * i + 2] != rr:
            bad.append((c.stream.name, "results", out[2 * i:2 * i + 2], rr))
        model[p.win[i]:p.win[i] + GRID_WIN] = want
    assert not bad, bad[:5]
    if p.dst != model:
        x = next(k for k in range(len(model)) if p.dst[k] != model[k])
        i = max(k for k in range(len(p.win)) if p.win[k] <= x)
        raise AssertionError(("bytes", streams[i].name, x - p.win[i]))
    assert len(cases) > 19 * 11 * 13 * 3 + 120


def test_inorder_more_streams_than_groups(rs, decode, monkeypatch):
    """1500 streams x 3 calls on the 1024-byte ring in step with the writer (pieces of 1 .. 300): more streams than a launch has lane
    groups, staged in chunks of 1 MiB of compressed bytes"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    from dstream_inorder_common import step_ring_stream
    rng = rng_for(101)
    data = book1()
    streams = [step_ring_stream(rs, rng, data, 1024, 1, 300, "#%d" % t, n_blocks=12) for t in range(1500)]
    cuts = [[4, 8, 12]] * len(streams)
    wants = [rs.decode(s, c) for s, c in zip(streams, cuts)]
    from dstream_common import run_placed
    bad = run_placed(streams, cuts, wants, decode, ("1500",))
    assert not bad, (len(bad), bad[:5])


def test_inorder_every_block_on_the_exact_layouts_and_the_hostile_list(rs, decode, every_block):
    """layouts a .. f and the hostile list with the knob at 1: results, states and bytes are the reference's"""
    rng = rng_for(102)
    streams = [s for s in layout_set(rs, rng, 6) if s.layout != "g"] + hostile_set(rs, rng, 4)
    bad, _ = check_set(rs, streams, 3, rng, decode, ("every",))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("every", [0, 1])
def test_inorder_equals_the_existing_call_where_no_slot_overlaps(amd, rs, decode, every):
    """layouts a .. f: out_len, states and every byte of the destination are lz4hip_decompress_safe_stream_batch's, call after call --
    with the knob at 0 (the same instances run) and at 1 (every block in order)"""
    rng = rng_for(103)
    streams = [s for s in layout_set(rs, rng, 8) if s.layout != "g"]
    cuts = padded_cuts(streams, 3, rng)
    a, b = Placed(streams, cuts), Placed(streams, cuts)
    old = lib_decoder(amd.lib())
    amd.set_option("dstream_inorder", every)
    try:
        for k in range(len(cuts[0])):
            ca, cb = a.call(k), b.call(k)
            ra, oa, na = decode(a.state, *ca[:4], a.dst, *ca[4:8])
            rb, ob, nb = old(b.state, *cb[:4], b.dst, *cb[4:8])
            assert ra == 0 and rb == 0 and oa == ob and na == nb, k
            a.state, b.state = [tuple(int(v) for v in s) for s in na], [tuple(int(v) for v in s) for s in nb]
            assert a.dst == b.dst, k
    finally:
        amd.set_option("dstream_inorder", 0)


def test_inorder_round_trip_from_compress_streams_on_a_ring_in_step(amd):
    """CompressStreams.compressAt on a ring of 4096 bytes, 16 streams x 10 calls of one 1000-byte block, decoded through
    DecodeStreams(inOrder=True) into a ring kept in step: every block comes back, the guards stand"""
    data = book1()
    n, bs, ring, calls = 16, 1000, 4096, 10
    cap = amd.maxCompressedLength(bs)
    arena = bytearray(n * ring)
    dst = bytearray([FILL]) * (n * (ring + GUARD) + GUARD)
    win = [GUARD + t * (ring + GUARD) for t in range(n)]
    pos, hend, hlen = [0] * n, [0] * n, [0] * n
    with amd.CompressStreams(n) as cs:
        ds = amd.DecodeStreams(n, inOrder=True)
        for call in range(calls):
            so, do = [], []
            for t in range(n):
                if pos[t] + bs > ring:
                    pos[t] = 0
                o = 5000 * t + call * bs
                arena[t * ring + pos[t]:t * ring + pos[t] + bs] = data[o:o + bs]
                so.append(t * ring + pos[t]); do.append(win[t] + pos[t])
            comp = bytearray(n * cap)
            out, cons = cs.compressAt(list(range(n)), bytes(arena), so, [bs] * n, list(range(n + 1)), hend, hlen, [t * ring for t in range(n)],
                                      [ring] * n, comp, [t * cap for t in range(n)], [cap] * n)
            assert all(r > 0 for r in out) and list(cons) == [bs] * n, (call, list(out)[:4])
            got = ds.decompress(list(range(n)), bytes(comp), [t * cap for t in range(n)], list(out), list(range(n + 1)), dst, do, [bs] * n, win, [ring] * n)
            assert list(got) == [bs] * n, (call, list(got)[:8])
            for t in range(n):
                o = 5000 * t + call * bs
                assert dst[do[t]:do[t] + bs] == data[o:o + bs], (call, t)
                hlen[t] = hlen[t] + bs if hend[t] == so[t] and hlen[t] else bs
                hend[t] = so[t] + bs
                pos[t] += bs
    for t in range(n):
        assert dst[win[t] - GUARD:win[t]] == bytes([FILL]) * GUARD
    assert dst[-GUARD:] == bytes([FILL]) * GUARD


def test_inorder_python_layer_and_two_threads(amd, rs):
    """DecodeStreams(inOrder=True) from two host threads on disjoint stream sets at once; a per-call inOrder=False on a set of streams
    none of whose slots overlaps alternates the two entry points"""
    def py_decode(ds, alternate):
        calls = [0]

        def f(state, src, so, sl, first, dst, do, dc, wo, wl):
            ids = list(range(len(state)))
            calls[0] += 1
            out = ds.decompress(ids, src, so, sl, first, dst, do, dc, wo, wl, inOrder=(False if alternate and calls[0] & 1 else None))
            return 0, list(out), ds.state()
        return f
    res = [None, None]

    def work(k):
        rng = rng_for(110 + k)
        if k == 0:
            streams = layout_streams(rs, rng, ("s", 4096, 1, 1000), 12) + layout_streams(rs, rng, ("m", "max", 1024, True), 6)
        else:
            streams = [s for s in layout_set(rs, rng, 4) if s.layout in "abde"]
        res[k] = check_set(rs, streams, 4, rng, py_decode(amd.DecodeStreams(len(streams), inOrder=True), k == 1), ("thread %d" % k,))[0]
    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert res[0] == [] and res[1] == [], (res[0][:3] if res[0] else None, res[1][:3] if res[1] else None)


def program_streams(rs):
    """a few overlap streams for the C++ and JNI programs, and one contiguous stream (alt: its calls alternate between the entry points)"""
    rng = rng_for(120)
    from dstream_common import make_stream
    out = [(s, False) for kind in (("s", 1024, 1, 300), ("s", 8192, 1, 1500), ("m", "fit", 1024, True), ("g",)) for s in layout_streams(rs, rng, kind, 1)]
    return out + [(make_stream(rs, "a", rng, book1(), tag="alt", zero_at_jump=False), True)]


def run_program(rs, exe, tmp_path, alt_arg):
    """every program stream cut into four calls; results, the state behind the last call, and the window against the replay of the
    reference's decoded bytes"""
    for s, alt in program_streams(rs):
        n = len(s.blocks)
        cuts = sorted({max(1, n // 4), max(1, n // 2), max(1, 3 * n // 4), n})
        w = rs.decode(s, cuts)
        name = "s.bin.alt" if alt and alt_arg is None else "s.bin"
        (tmp_path / name).write_bytes(stream_file(s, cuts))
        args = [exe, str(tmp_path / name), str(tmp_path / "w.bin")] + (["alt"] if alt and alt_arg else [])
        p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (s.name, p.returncode, p.stderr.decode()[-2000:])
        lines = p.stdout.decode().splitlines()
        assert [int(v) for v in lines[0].split()] == w.out, (s.name, lines[0][:80], w.out[:8])
        assert same_state(tuple(int(v) for v in lines[1].split()), w.states[-1]), (s.name, lines[1], w.states[-1])
        model = bytearray([FILL]) * s.win_len
        for b, r, by in zip(s.blocks, w.out, w.data):
            model[b.off:b.off + max(r, 0)] = by
        assert (tmp_path / "w.bin").read_bytes() == bytes(model), s.name
        yield s, p.stdout.decode()


def test_inorder_cpp_mirror(rs, tmp_path):
    """tests/cpp/dstream_inorder_mirror_test.cpp: DecodeStreams(3, true) of host/lz4hip.hpp, a stream in four calls"""
    exe = build_mirror("dstream_inorder_mirror_test", tmp_path)
    assert len(list(run_program(rs, exe, tmp_path, "alt"))) == 5


def test_inorder_jni_program(rs, tmp_path):
    """tests/jni_stub/fake_jni_dstream_inorder.c: the JNI shim's LZ4HIP_batchSafeStreamInOrder over the fake JNIEnv"""
    exe = build_fake_jni("fake_jni_dstream_inorder", tmp_path)
    for s, text in run_program(rs, exe, tmp_path, None):
        assert "checks ok" in text, s.name


def test_inorder_ring_size_python(amd):
    assert amd.decoderRingBufferSize(4096) == ring_size(4096) and amd.decoderRingBufferSize(-1) == 0


def test_inorder_multidev_host_path_on_one_gpu():
    """lz4hip_init([0] * 2): the host call takes the multi-device branch (whole streams per listed device)"""
    assert "dstream inorder multidev ok D=2" in run_child("dstream_inorder_multidev_child.py", "2", "repeat", timeout=600)
