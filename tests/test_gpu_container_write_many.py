"""Many LZ4 Frames / LZ4Block streams WRITTEN in one call (-m gpu): lz4hip_container_blocks_many against the pure-Python writers over the
reference-backed engine per item and, separately, against lz4hip_container_blocks called per item -- the contract is that call, item by
item.  The items are the case list of tests/container_write_many_common.py; nothing provokes a fault."""
import importlib
import io
import random
import threading

import pytest

import container_write_many_common as wm
import streams_common as sc

pytestmark = pytest.mark.gpu
KINDS = (wm.FRAME, wm.LZ4BLOCK)
LEVELS = (0, 9, 4)
_SINGLE = {}


@pytest.fixture(scope="module")
def S(amd):
    return importlib.import_module("lz4-java_amd.streams")


def items_of(O, corpus, kind):
    return wm.for_kind(wm.cases(O, corpus), kind)


def single(amd, O, corpus, kind, level):
    """lz4hip_container_blocks per item, once per (kind, level)"""
    if (kind, level) not in _SINGLE:
        _SINGLE[kind, level] = [amd.LZ4HIPBatch.containerBlocks(kind, d, bs, cks, level) for (_, d, bs, cks, _, _, _) in items_of(O, corpus, kind)]
    return _SINGLE[kind, level]


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("kind", KINDS)
def test_case_list_in_one_call(amd, S, ref, O, corpus, kind, level):
    """5. the whole case list in one call: each item equals the oracle's bytes and, separately, the single call's; gap bytes are zero,
    content hashes the reference's XXH32, guard bytes behind item_dst_off[n] intact (write_many checks those)"""
    items, want = items_of(O, corpus, kind), wm.oracle_items(S, ref, O, corpus, kind, level)
    got = wm.write_many(amd.lib(), kind, level, items)
    wm.same_items(got, want, items, "oracle")
    one = single(amd, O, corpus, kind, level)
    for (gb, _), ob, it in zip(got, one, items):
        assert gb == ob, ("single call", it[0], len(gb), len(ob))
    assert any(it[6] for it in items) and not all(it[6] for it in items)


@pytest.mark.parametrize("kind", KINDS)
def test_shuffled_scattered_and_one_item_per_call(amd, S, ref, O, corpus, kind):
    """6. the items in shuffled order, with out-of-order and overlapping sources, and one item per call: no result changes"""
    items, want = items_of(O, corpus, kind), wm.oracle_items(S, ref, O, corpus, kind, 0)
    order = list(range(len(items)))
    random.Random(5).shuffle(order)
    wm.same_items(wm.write_many(amd.lib(), kind, 0, [items[i] for i in order]), [want[i] for i in order], [items[i] for i in order], "shuffled")
    assert wm.Packed(items, scatter=True).overlaps >= 3
    wm.same_items(wm.write_many(amd.lib(), kind, 0, items, scatter=True), want, items, "scattered")
    for i in range(0, len(items), 3):
        wm.same_items(wm.write_many(amd.lib(), kind, 0, [items[i]]), [want[i]], [items[i]], "alone")


@pytest.mark.parametrize("kind", KINDS)
def test_small_staging_chunks_make_groups(amd, S, ref, O, corpus, kind, monkeypatch):
    """7. LZ4HIP_HOST_CHUNK_MB=1 (read per call): 3000 small items, the case list among them, and an item larger than a group: every
    result is as in one group"""
    text = corpus["book1[:200000]"]
    rng = random.Random(13)
    cases, want_cases = items_of(O, corpus, kind), wm.oracle_items(S, ref, O, corpus, kind, 0)
    small = []
    for i in range(3000 - len(cases)):
        o = rng.randrange(len(text) - 1200)
        d = text[o:o + 300 + i % 700] if i % 7 else rng.randbytes(100 + i % 300)
        small.append(("s%d" % i, d, (64, 1000, 65536)[i % 3], kind == 0 and i % 2 == 0, wm.GAPS[i % 3], wm.GAPS[(i // 3) % 3], i % 4 == 0))
    big = ("big", (text * 9)[:(1 << 20) + 70001], 65536, kind == 0, 7, 19, True)
    items = small[:1000] + cases + small[1000:2000] + [big] + small[2000:]
    assert len(items) == 3001 and sum((len(it[1]) + 15) & ~15 for it in items) > 3 << 20
    one_group = wm.write_many(amd.lib(), kind, 0, items)
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    groups = wm.write_many(amd.lib(), kind, 0, items)
    assert groups == one_group
    wm.same_items(groups[1000:1000 + len(cases)], want_cases, cases, "groups")
    eng = wm.oracle_engine(ref, O)
    for i in list(range(0, 3001, 97)) + [999, 2000 + len(cases), 3000]:
        name, d, bs, cks, _, _, h = items[i]
        assert groups[i] == (wm.writer_blocks(S, eng, kind, d, bs, cks), ref.xxh32(d, 0) if h else 0), name


@pytest.mark.parametrize("kind", KINDS)
def test_many_small_payloads_at_large_block_sizes(amd, S, ref, O, corpus, kind):
    """7b. the shape the call is for: thousands of payloads far smaller than their block size.  The case list's payloads and 3000
    payloads of 40 .. 1100 bytes at block sizes of 4 MiB and 32 MiB in one call.  The case list's items and every tenth of the others
    are the oracle's bytes (the writers allocate a block size's bound per payload: megabytes each, so not all 3000), a sample the single
    call's, and EVERY item reads back as its payload through lz4hip_container_decode_many with the content hash the reference's.
    Compress slots are sized by what an item holds (container_write_rules.h item_slot_bytes): by the block size they would be 30 GiB
    of device scratch here"""
    text = corpus["book1[:200000]"]
    rng = random.Random(29)
    items = [(n, d, 4 << 20, cks, gh, gt, h) for (n, d, _, cks, gh, gt, h) in items_of(O, corpus, kind)]
    n_cases = len(items)
    for i in range(3000):
        o = rng.randrange(len(text) - 1200)
        d = text[o:o + 40 + (i * 37) % 1060] if i % 5 else rng.randbytes(40 + i % 200)
        items.append(("small%d" % i, d, (32 << 20) if i % 4 == 0 else (4 << 20), kind == 0 and i % 2 == 0, wm.GAPS[i % 3], wm.GAPS[(i // 3) % 3], i % 4 == 1))
    nb, need = wm.bound_many(amd.lib(), kind, wm.Packed(items))
    assert int(nb.sum()) == sum(1 for it in items if it[1]) and sum(int(it[2]) for it in items) > 30 << 30
    got = wm.write_many(amd.lib(), kind, 0, items)
    eng = wm.oracle_engine(ref, O)
    some = list(range(n_cases)) + list(range(n_cases, len(items), 10))
    want = [(wm.writer_blocks(S, eng, kind, items[i][1], items[i][2], items[i][3]), ref.xxh32(items[i][1], 0)) for i in some]
    wm.same_items([got[i] for i in some], want, [items[i] for i in some], "large block sizes")
    bodies = wm.read_back_bodies(kind, items, [g[0] for g in got])
    # (the reader sizes its destination by the block maximum it is told: the payload's length is one that holds here)
    back = amd.LZ4HIPBatch.containerDecodeMany(kind, bodies, [max(64, len(it[1])) for it in items], 4, [it[3] for it in items])
    for it, body, g, (data, sizes, consumed, why, code) in zip(items, bodies, got, back):
        assert (data, consumed, why, code) == (it[1], len(body), 0, 0) and g[1] == (ref.xxh32(it[1], 0) if it[6] else 0), it[0]
    for i in list(range(0, len(items), 211)) + [len(items) - 1]:
        assert got[i][0] == amd.LZ4HIPBatch.containerBlocks(kind, items[i][1], items[i][2], items[i][3], 0), items[i][0]


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_through_the_many_read(amd, S, O, corpus, kind):
    """8. everything written goes back through lz4hip_container_decode_many"""
    items = items_of(O, corpus, kind)
    for level in (0, 9):
        got = wm.write_many(amd.lib(), kind, level, items)
        bodies = wm.read_back_bodies(kind, items, [g[0] for g in got])
        back = amd.LZ4HIPBatch.containerDecodeMany(kind, bodies, [it[2] for it in items], 64, [it[3] for it in items])
        for it, body, (data, sizes, consumed, why, code) in zip(items, bodies, back):
            assert (data, consumed, why, code) == (it[1], len(body), 0, 0), it[0]
            assert sizes == [n for _, n in wm.block_table(len(it[1]), it[2])], it[0]


@pytest.mark.skipif(sc.LZ4_CLI is None, reason="no lz4 command line on this machine")
def test_the_lz4_command_line_reads_the_frames_the_device_wrote(amd, S, O, corpus):
    """8b. the CLI reads the frames written on the device"""
    payloads = [it[1] for it in wm.cases(O, corpus)]
    B = S.FLG.Bits
    for bits in ((B.BLOCK_INDEPENDENCE,), (B.BLOCK_INDEPENDENCE, B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, B.CONTENT_SIZE)):
        frames = S.writeFrames(payloads, blockSize=S.BLOCKSIZE.SIZE_64KB, bits=bits)
        assert sc.cli(["-d"], b"".join(frames)) == b"".join(payloads)


def test_two_host_threads_at_once(amd, S, ref, O, corpus):
    """9. two host threads, a call each, at the same time"""
    res, err = {}, []

    def work(kind):
        try:
            for _ in range(3):
                res[kind] = wm.write_many(amd.lib(), kind, 0, items_of(O, corpus, kind))
        except BaseException as e:   # noqa: BLE001 -- handed to the main thread
            err.append(e)
    want = {k: wm.oracle_items(S, ref, O, corpus, k, 0) for k in KINDS}
    th = [threading.Thread(target=work, args=(k,)) for k in KINDS]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for k in KINDS:
        wm.same_items(res[k], want[k], items_of(O, corpus, k), "threads")


def _alone(make, p):
    sink = io.BytesIO()
    w = make(sink)
    w.write(p)
    w.close()
    return sink.getvalue()


@pytest.mark.parametrize("hc", [None, 9])
def test_write_frames_and_block_streams_equal_the_per_payload_writers(amd, S, O, corpus, hc):
    """10. streams.writeFrames / writeBlockStreams on the real engine against LZ4FrameOutputStream / LZ4BlockOutputStream per payload"""
    payloads = [it[1] for it in wm.cases(O, corpus)]
    engine = S.HIPEngine(hc)
    B = S.FLG.Bits
    for bits in ((B.BLOCK_INDEPENDENCE,), (B.BLOCK_INDEPENDENCE, B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, B.CONTENT_SIZE), (B.BLOCK_INDEPENDENCE, B.CONTENT_CHECKSUM)):
        want = [_alone(lambda f: S.LZ4FrameOutputStream(f, S.BLOCKSIZE.SIZE_64KB, len(p) if B.CONTENT_SIZE in bits else -1, *bits, engine=engine), p) for p in payloads]
        assert S.writeFrames(payloads, engine=engine, blockSize=S.BLOCKSIZE.SIZE_64KB, bits=bits) == want, bits
    assert S.readFrames(want) == [(p, None) for p in payloads]
    for bs in (64, 1025, 65536):
        some = [p for p in payloads if len(p) <= 40 * bs]
        want = [_alone(lambda f: S.LZ4BlockOutputStream(f, bs, engine=engine), p) for p in some]
        assert S.writeBlockStreams(some, engine=engine, blockSize=bs) == want, bs
        assert S.readBlockStreams(want) == [(p, None) for p in some]


@pytest.mark.parametrize("kind", KINDS)
def test_cpp_mirror_program(amd, S, ref, O, corpus, kind, tmp_path):
    """11a. BatchEngine::containerBlocksMany of the C++ host mirror over the case list"""
    from support import build_mirror
    exe = build_mirror("container_write_many_mirror_test", tmp_path, werror=True)
    items = items_of(O, corpus, kind)
    wm.same_items(wm.run_program(exe, tmp_path, kind, 0, items), wm.oracle_items(S, ref, O, corpus, kind, 0), items, "C++ mirror")


def test_cpp_write_frames_and_block_streams(amd, S, O, corpus, tmp_path):
    """11b. writeFrames / writeBlockStreams of the C++ host mirror equal the Python ones (the program compares each container with the
    C++ per-payload writer itself)"""
    from support import build_mirror
    exe = build_mirror("container_write_many_mirror_test", tmp_path, werror=True)
    payloads = [it[1] for it in wm.cases(O, corpus)]
    B = S.FLG.Bits
    got = wm.run_program_streams(exe, tmp_path, 0, 4, 0x1C, payloads)
    assert got == S.writeFrames(payloads, blockSize=S.BLOCKSIZE.SIZE_64KB, bits=(B.BLOCK_INDEPENDENCE, B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, B.CONTENT_SIZE))
    got = wm.run_program_streams(exe, tmp_path, 0, 4, 0, payloads)
    assert got == S.writeFrames(payloads, blockSize=S.BLOCKSIZE.SIZE_64KB)
    got = wm.run_program_streams(exe, tmp_path, 1, 1025, 0, payloads)
    assert got == S.writeBlockStreams(payloads, blockSize=1025)


@pytest.mark.parametrize("kind", KINDS)
def test_fake_jni_program(amd, S, ref, O, corpus, kind, tmp_path):
    """11c. LZ4HIPJNI.LZ4HIP_containerBlocksMany / ..ManyBound of the JNI shim over the fake JNIEnv, on the case list"""
    from support import build_fake_jni
    exe = build_fake_jni("fake_jni_container_write_many", tmp_path)
    items = items_of(O, corpus, kind)
    wm.same_items(wm.run_program(exe, tmp_path, kind, 9, items, jni=True), wm.oracle_items(S, ref, O, corpus, kind, 9), items, "fake JNI")
