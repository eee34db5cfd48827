"""Many LZ4 Frame bodies / LZ4Block streams in ONE call (-m gpu): lz4hip_container_decode_many against the reference-backed restatement
of the read path (streams_common.OracleDeviceEngine, on liblz4 1.9.3 and its XXH32) per item and, separately, against
lz4hip_container_decode called per item -- the contract is that call, item by item.  The items are the case list of
tests/container_many_common.py: hostile inputs here are inputs whose results the reference defines; nothing provokes a fault."""
import random
import threading

import pytest

import container_many_common as cm
import streams_common as sc

pytestmark = pytest.mark.gpu
KINDS = (cm.FRAME, cm.LZ4BLOCK)
_ORACLE, _SINGLE = {}, {}


@pytest.fixture(scope="module")
def case_list(ref, corpus):
    return cm.cases(ref, corpus)


def oracle(ref, O, case_list, kind, n_max):
    """computed once per (kind, n_max), shared and left unchanged"""
    if (kind, n_max) not in _ORACLE:
        _ORACLE[kind, n_max] = cm.oracle_results(sc.OracleDeviceEngine(ref, O), cm.of_kind(case_list, kind), n_max)
    return _ORACLE[kind, n_max]


def single(amd, case_list, kind, n_max):
    """lz4hip_container_decode per item, once per (kind, n_max)"""
    if (kind, n_max) not in _SINGLE:
        _SINGLE[kind, n_max] = [tuple(amd.LZ4HIPBatch.containerDecode(k, body, mb, n_max, cks)) for (_, k, body, mb, cks) in cm.of_kind(case_list, kind)]
    return _SINGLE[kind, n_max]


def same(got, want, items, tag):
    assert len(got) == len(want) == len(items)
    for g, w, it in zip(got, want, items):
        assert tuple(g) == tuple(w), (tag, it[0], g[1:], w[1:])


@pytest.mark.parametrize("n_max", [2, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_case_list_in_one_call(amd, ref, O, case_list, kind, n_max):
    """1. the whole case list in one call per kind: against the reference-backed oracle, and against the single call, per item; guard
    bytes behind item_dst_off[n] and the sizes entries behind item_first[n] stay (decode_many checks both)"""
    items = cm.of_kind(case_list, kind)
    got = cm.decode_many(amd.lib(), kind, items, n_max, pad=5)
    same(got, oracle(ref, O, case_list, kind, n_max), items, "oracle")
    same(got, single(amd, case_list, kind, n_max), items, "single call")
    whys = {g[3] for g in got}
    assert whys >= ({0, 1, 2, 3, 4, 5, 7} if kind == 0 else {0, 1, 2, 3, 6, 7}) - ({7} if n_max == 64 else set()), whys


@pytest.mark.parametrize("kind", KINDS)
def test_shuffled_and_failing_items_between_good_ones(amd, ref, O, case_list, kind):
    """2. the same items in shuffled order, and each failing item between two good ones: every result is unchanged"""
    items, want = cm.of_kind(case_list, kind), oracle(ref, O, case_list, kind, 64)
    order = list(range(len(items)))
    random.Random(5).shuffle(order)
    got = cm.decode_many(amd.lib(), kind, [items[i] for i in order], 64)
    same(got, [want[i] for i in order], [items[i] for i in order], "shuffled")
    good = next(i for i, (it, w) in enumerate(zip(items, want)) if w[3] == 0 and len(w[1]) == 3)
    failing = [i for i, w in enumerate(want) if w[3] in (2, 3, 4, 5, 6)]
    assert len(failing) > 100
    mixed = [good]
    for i in failing:
        mixed += [i, good]
    got = cm.decode_many(amd.lib(), kind, [items[i] for i in mixed], 64)
    same(got, [want[i] for i in mixed], [items[i] for i in mixed], "between good ones")


@pytest.mark.parametrize("kind", KINDS)
def test_call_of_one_item_equals_the_single_call(amd, case_list, kind):
    """3. one item per call"""
    items, want = cm.of_kind(case_list, kind), single(amd, case_list, kind, 2)
    picks = [i for i, it in enumerate(items) if "cut" not in it[0]] + [i for i, it in enumerate(items) if "cut" in it[0]][::37]
    for i in picks:
        assert cm.decode_many(amd.lib(), kind, [items[i]], 2)[0] == want[i], items[i][0]
    assert amd.LZ4HIPBatch.containerDecodeMany(kind, [items[picks[3]][2]], [items[picks[3]][3]], 2, [items[picks[3]][4]]) == [want[picks[3]]]


def test_ten_thousand_one_block_frames(amd, ref, corpus):
    """4. 10000 one-block frames of about 200 bytes in one call"""
    text = corpus["book1[:200000]"]
    rng = random.Random(9)
    blocks = []
    for i in range(10000):
        o = rng.randrange(len(text) - 400)
        blocks.append(text[o:o + 300 + i % 90] if i % 7 else rng.randbytes(150 + i % 90))     # (every seventh: raw)
    items = [("f%d" % i, 0, cm.frame_body(ref, [b], i % 3 == 0, i % 2 == 0), 65536, i % 3 == 0) for i, b in enumerate(blocks)]
    assert 150 < sum(len(it[2]) for it in items) / len(items) < 350
    got = cm.decode_many(amd.lib(), 0, items, 4)
    for i, (g, b) in enumerate(zip(got, blocks)):
        assert g == (b, [len(b)], len(items[i][2]), 0 if i % 2 == 0 else 1, 0), i


@pytest.mark.parametrize("kind", KINDS)
def test_small_staging_chunks_make_groups(amd, ref, O, corpus, case_list, kind, monkeypatch):
    """5. LZ4HIP_HOST_CHUNK_MB=1 (read per call): the case list and enough 64 KiB raw items to need three groups"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    rng = random.Random(11)
    items, want = list(cm.of_kind(case_list, kind)), list(oracle(ref, O, case_list, kind, 64))
    for i in range(40):
        b = rng.randbytes(65536)
        body = cm.frame_body(ref, [b], True) if kind == 0 else cm.block_stream(ref, [b], 65536)
        at = rng.randrange(len(items) + 1)
        items.insert(at, ("big%d" % i, kind, body, 65536, kind == 0))
        want.insert(at, (b, [65536], len(body), 0, 0))
    assert sum((len(it[2]) + 15) & ~15 for it in items) > 3 << 20
    same(cm.decode_many(amd.lib(), kind, items, 64), want, items, "groups")


@pytest.mark.parametrize("batch", [2, None])
def test_read_frames_and_block_streams_equal_the_sequential_readers(amd, ref, corpus, case_list, batch):
    """7. streams.readFrames / readBlockStreams against LZ4FrameInputStream / LZ4BlockInputStream per item: the case list wrapped in
    frame headers, concatenated and skippable frames, a wrong content checksum, a wrong content size, a linked-block frame"""
    import importlib
    S = importlib.import_module("lz4-java_amd.streams")
    frames, streams = cm.stream_items(ref, corpus, case_list)
    kw = {} if batch is None else {"batchBlocks": batch}
    cm.same_reads(S.readFrames(frames, **kw), [cm.read_sequentially(lambda f: S.LZ4FrameInputStream(f, **kw), it) for it in frames], "frames")
    cm.same_reads(S.readBlockStreams(streams, **kw), [cm.read_sequentially(lambda f: S.LZ4BlockInputStream(f, **kw), it) for it in streams], "block streams")


@pytest.mark.parametrize("kind", KINDS)
def test_cpp_mirror_program(amd, ref, O, case_list, kind, tmp_path):
    """8. BatchEngine::containerDecodeMany of the C++ host mirror over the case list"""
    from support import build_mirror
    exe = build_mirror("container_many_mirror_test", tmp_path, werror=True)
    items = cm.of_kind(case_list, kind)
    same(cm.run_mirror(exe, tmp_path, items, 64), oracle(ref, O, case_list, kind, 64), items, "C++ mirror")


@pytest.mark.parametrize("batch", [2, 64])
def test_cpp_read_frames_and_block_streams(amd, ref, corpus, case_list, batch, tmp_path):
    """8b. readFrames / readBlockStreams of the C++ host mirror: rounds, concatenated and skippable frames, content size and checksum.
    The program compares every item with the C++ sequential reader; here the bytes, and the message of every IOException /
    EOFException, are compared with the Python sequential readers' too"""
    import importlib
    from support import build_mirror
    S = importlib.import_module("lz4-java_amd.streams")
    exe = build_mirror("container_many_mirror_test", tmp_path, werror=True)
    frames, streams = cm.stream_items(ref, corpus, case_list)
    for kind, items, reader in ((0, frames, S.LZ4FrameInputStream), (1, streams, S.LZ4BlockInputStream)):
        got = cm.run_mirror_streams(exe, tmp_path, kind, items, batch)
        want = [cm.read_sequentially(lambda f: reader(f, batchBlocks=batch), it) for it in items]
        for i, ((gd, gc, gm), (wd, we)) in enumerate(zip(got, want)):
            assert gd == wd and (gc is None) == (we is None), (kind, i, gc, gm, we)
            if type(we).__name__ in ("IOException", "EOFException"):
                assert (gc, gm) == (type(we).__name__, str(we)), (kind, i, gc, gm, we)
        assert {c for _, c, _ in got} >= {None, "IOException"}


@pytest.mark.parametrize("kind", KINDS)
def test_fake_jni_program(amd, ref, O, case_list, kind, tmp_path):
    """9. LZ4HIPJNI.LZ4HIP_containerDecodeMany / ..ManyBound of the JNI shim over the fake JNIEnv, on the case list"""
    from support import build_fake_jni
    exe = build_fake_jni("fake_jni_container_many", tmp_path)
    items = cm.of_kind(case_list, kind)
    same(cm.run_fake_jni(exe, tmp_path, items, 64), oracle(ref, O, case_list, kind, 64), items, "fake JNI")


def test_two_host_threads_at_once(amd, ref, O, case_list):
    """6. two host threads, a call each, at the same time"""
    res, err = {}, []

    def work(kind):
        try:
            for _ in range(3):
                res[kind] = cm.decode_many(amd.lib(), kind, cm.of_kind(case_list, kind), 64)
        except BaseException as e:   # noqa: BLE001 -- handed to the main thread
            err.append(e)
    want = {k: oracle(ref, O, case_list, k, 64) for k in KINDS}
    th = [threading.Thread(target=work, args=(k,)) for k in KINDS]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for k in KINDS:
        same(res[k], want[k], cm.of_kind(case_list, k), "threads")
