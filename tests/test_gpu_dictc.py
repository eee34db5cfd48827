"""The dictionary compressor (LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream, external dictionary) on the GPU against the
reference library's own functions: the shared set of tests/dictc_common.py through the host batch, per dictionary, in batches of 1 / 63 /
64 / 65 / 3000 records; the hand-built cases; one device batch of mixed sizes with 256 guard bytes round every slot; coalesced single
calls from eight threads on two handles; round trips through both dictionary decoders; the empty dictionary against the plain
compressor; the C++ mirror, the JNI shim and the multi-device host path."""
import ctypes as C
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from dictc_common import (BIG, DICT_LENS, RefDict, big_record, book1, book_records, bound, caps_for, dict_cuts, hand_cases, other_records,
                          parse, ref_compress, rng_for)
from support import build_fake_jni, build_mirror, run_child

pytestmark = pytest.mark.gpu
GUARD = 8


@pytest.fixture(scope="module")
def rd(ref):
    return RefDict(ref)


@pytest.fixture(scope="module")
def shared(O, corpus):
    """the records every dictionary gets (those cut out of the dictionary are added per dictionary)"""
    return book_records() + other_records(O, corpus) + [big_record(O)]


def rows_for(rd, d, recs):
    """[(record, capacity)] and the reference's (value, bytes) per row: the bound, the exact size, one byte less, 1 and 0"""
    rs, want = [], []
    for name, rec in recs:
        full = ref_compress(rd, d, rec)
        for cap in caps_for(len(rec), full[0], True):
            rs.append((rec, cap))
            want.append(full if cap >= full[0] else ref_compress(rd, d, rec, cap))
    return rs, want


def layout(rs):
    """one source buffer, one destination buffer with GUARD bytes in front of, between and behind the slots"""
    so, do, p, q = [], [], 0, GUARD
    for s, c in rs:
        so.append(p); do.append(q); p += len(s); q += c + GUARD
    return b"".join(s for s, _ in rs) + b"\0", so, do, q


def check(rs, want, got, dst, do, what, exact_tail):
    """values, bytes, and 0xEE everywhere outside the slots (exact_tail: behind the compressed bytes too -- the host path hands back
    exactly those)"""
    dst = bytes(dst)
    assert dst[:GUARD] == b"\xee" * GUARD, (what, "written in front of the first slot")
    for i, ((s, c), (r, by)) in enumerate(zip(rs, want)):
        assert int(got[i]) == r, (what, i, len(s), c, int(got[i]), r)
        o = do[i]
        assert dst[o:o + r] == by, (what, "bytes", i, len(s), c)
        tail = dst[o + (r if exact_tail else c):o + c + GUARD]
        assert tail == b"\xee" * len(tail), (what, "written outside the slot", i, len(s), c)


def host_batch(amd, handle, rs):
    src, so, do, q = layout(rs)
    dst = bytearray(b"\xee" * q)
    got = amd.LZ4HIPBatch.compressDict(src, so, [len(s) for s, _ in rs], dst, do, [c for _, c in rs], handle)
    return got, dst, do


@pytest.mark.parametrize("L", DICT_LENS)
def test_dictc_host_batches(amd, rd, shared, L):
    """the set against book1[:L] through the host batch: 3000 records (the set, its small records again until the batch is full), and
    batches of 1 / 63 / 64 / 65 out of it"""
    d = book1()[:L]
    rng = rng_for(300 + L)
    rs, want = rows_for(rd, d, shared + dict_cuts(L, rng))
    small = [i for i, (s, c) in enumerate(rs) if len(s) <= 4096]
    idx = list(range(len(rs)))
    while len(idx) < 3000:
        idx.append(small[(len(idx) * 7) % len(small)])
    rng.shuffle(idx)
    batches = [idx]
    for size in (1, 63, 64, 65):
        k = rng.randrange(0, len(idx) - size)
        batches.append(idx[k:k + size])
    batches.append([i for i in range(len(rs)) if len(rs[i][0]) == BIG][:1])   # (the 1 MiB + 3 block alone)
    with amd.LZ4Dictionary(d) as handle:
        for ids in batches:
            r2, w2 = [rs[i] for i in ids], [want[i] for i in ids]
            got, dst, do = host_batch(amd, handle, r2)
            check(r2, w2, got, dst, do, "host batch of %d, L=%d" % (len(ids), L), exact_tail=True)


def test_dictc_hand_built_cases(amd, rd):
    """the hand-built cases, each against its own random dictionary: the reference's output holds the intended sequence, and the
    engine's bytes are the reference's at every capacity"""
    groups = {}
    for c in hand_cases():
        groups.setdefault(c[1], []).append(c)
    assert len(groups) >= 5
    for d, cases in groups.items():
        for c in cases:
            c[3](parse(ref_compress(rd, d, c[2])[1]))
        rs, want = rows_for(rd, d, [(c[0], c[2]) for c in cases])
        with amd.LZ4Dictionary(d) as handle:
            got, dst, do = host_batch(amd, handle, rs)
        check(rs, want, got, dst, do, "hand-built, dictionary of %d" % len(d), exact_tail=True)


def test_dictc_device_batch_mixed_sizes_and_guards(amd, rd, shared):
    """one device batch, 0 bytes to 1 MiB + 3, 256 guard bytes round every slot: the guards do not change; every fifth capacity is one
    byte short and gives 0"""
    import torch
    G = 256
    d = book1()[:65536]
    rng = rng_for(17)
    recs = [rec for _, rec in shared + dict_cuts(65536, rng)]
    rng.shuffle(recs)
    full = [ref_compress(rd, d, rec) for rec in recs]
    caps = [(f[0] - 1) if i % 5 == 4 else rng.choice([bound(len(rec)), f[0], f[0] + 1]) for i, (rec, f) in enumerate(zip(recs, full))]
    want = [(0, b"") if i % 5 == 4 else f for i, f in enumerate(full)]
    assert all(ref_compress(rd, d, recs[i], caps[i])[0] == 0 for i in range(4, len(recs), 5))   # (the reference says 0 there too)
    assert min(len(r) for r in recs) == 0 and max(len(r) for r in recs) == BIG
    so, do, p, q = [], [], 0, G
    for rec, c in zip(recs, caps):
        so.append(p); do.append(q); p += len(rec); q += c + G
    dev = torch.device("cuda", 0)
    d_src = torch.frombuffer(bytearray(b"".join(recs) + b"\0"), dtype=torch.uint8).to(dev)
    d_dst = torch.full((q,), 0xEE, dtype=torch.uint8, device=dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    out = torch.full((len(recs),), -12345, dtype=torch.int32, device=dev)
    with amd.LZ4Dictionary(d) as handle:
        for _ in range(2):   # (the second call finds the handle's table image in place)
            out.fill_(-12345); d_dst.fill_(0xEE)
            amd.DeviceBatch.compress_dict(d_src, i64(so), i32([len(r) for r in recs]), d_dst, i64(do), i32(caps), out, handle)
            torch.cuda.synchronize()
            got, dst = out.cpu().tolist(), d_dst.cpu().numpy().tobytes()
            assert dst[:G] == b"\xee" * G
            for i, (r, by) in enumerate(want):
                assert got[i] == r, (i, len(recs[i]), caps[i], got[i], r)
                assert dst[do[i]:do[i] + r] == by, ("bytes", i, len(recs[i]))
                assert dst[do[i] + caps[i]:do[i] + caps[i] + G] == b"\xee" * G, ("guard behind slot", i, len(recs[i]), caps[i])


def test_dictc_single_calls_from_eight_threads_on_two_handles(amd, rd):
    """single calls coalesce per handle: eight threads alternate between two dictionaries, every call gets its own dictionary's bytes"""
    b = book1()
    rng = rng_for(18)
    da, db = b[:4096], b[:65537]
    recs = []
    for _ in range(120):
        n = rng.choice([0, 12, 13, 64, 300, 1000, 4096])
        o = rng.randrange(200000, len(b) - n)
        recs.append(b[o:o + n])
    recs += [x for _, x in dict_cuts(4096, rng)]
    jobs = [(d, h, rec) for rec in recs for d, h in ((da, 0), (db, 1))]
    want = [ref_compress(rd, d, rec) for d, h, rec in jobs]
    handles = [amd.LZ4Dictionary(da), amd.LZ4Dictionary(db)]
    c = amd.LZ4Factory.hipInstance().fastCompressor()

    def one(job):
        d, h, rec = job
        buf = bytearray(b"\xee" * (bound(len(rec)) + GUARD + 3))
        r = c.compressWithDict(handles[h], rec, 0, len(rec), buf, 3, bound(len(rec)))
        return r, buf

    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, jobs))
    assert len(jobs) > 200
    for (d, h, rec), (r, buf), (wr, wb) in zip(jobs, res, want):
        assert r == wr and bytes(buf[3:3 + r]) == wb, (len(d), len(rec), r, wr)
        assert bytes(buf[3 + r:]) == b"\xee" * (len(buf) - 3 - r) and buf[:3] == b"\xee\xee\xee"
    # a capacity one byte short is the compressor's exception, and writes nothing past the slot
    rec = recs[5]
    wr = ref_compress(rd, da, rec)[0]
    buf = bytearray(b"\xee" * (wr + GUARD))
    with pytest.raises(amd.LZ4Exception, match="maxDestLen is too small"):
        c.compressWithDict(handles[0], rec, 0, len(rec), buf, 0, wr - 1)
    assert bytes(buf[wr - 1:]) == b"\xee" * (GUARD + 1)
    assert c.compressWithDict(handles[0], rec) == ref_compress(rd, da, rec)[1]
    for h in handles:
        h.close()


def test_dictc_round_trips(amd, rd):
    """records compressed here decode back to the input through lz4hip_decompress_safe_dict_batch and through the reference's
    LZ4_decompress_safe_usingDict; most of them reach into the dictionary"""
    b = book1()
    rng = rng_for(19)
    for L in (9, 4096, 65536, 100000):
        d = b[:L]
        recs = []
        for _ in range(200):
            n = rng.choice([13, 64, 300, 1000, 4096, 20000])
            o = rng.randrange(200000, len(b) - n)
            recs.append(b[o:o + n])
        recs += [x for _, x in dict_cuts(L, rng)] + [b[200000:270000]]
        rs = [(rec, bound(len(rec))) for rec in recs]
        with amd.LZ4Dictionary(d) as handle:
            got, dst, do = host_batch(amd, handle, rs)
            streams = [bytes(dst[o:o + r]) for o, r in zip(do, got)]
            assert all(r > 0 for r in got)
            back_rs = [(s, len(rec)) for s, rec in zip(streams, recs)]
            src, so, do2, q = layout(back_rs)
            back = bytearray(b"\xee" * q)
            r2 = amd.LZ4HIPBatch.decompressSafeDict(src, so, [len(s) for s in streams], back, do2, [len(rec) for rec in recs], handle)
        for i, rec in enumerate(recs):
            assert r2[i] == len(rec) and bytes(back[do2[i]:do2[i] + len(rec)]) == rec, (L, i, len(rec))
            assert rd.decode(streams[i], len(rec), d) == (len(rec), rec), (L, i, len(rec))
        if L >= 4096:
            uses = sum(any(off > pos for pos, off, ml in parse(s)) for s, rec in zip(streams, recs) if len(rec) >= 300)
            assert uses >= 0.9 * sum(len(rec) >= 300 for rec in recs), (L, uses)


def test_dictc_empty_dictionary_and_the_plain_compressor(amd, rd, ref):
    """from 65547 bytes on the empty dictionary gives lz4hip_compress_fast's bytes; below, byU32 at every size, mostly other bytes (as
    the reference does); dictionaries of 1 and 7 bytes are the empty dictionary"""
    b = book1()
    rng = rng_for(20)
    big = [b[200000:200000 + n] for n in (65547, 65548, 70000, 200000)]
    small = []
    for _ in range(100):
        n = rng.randrange(64, 4097)
        o = rng.randrange(200000, len(b) - n)
        small.append(b[o:o + n])
    rs = [(rec, bound(len(rec))) for rec in big + small]
    src, so, do, q = layout(rs)
    plain_dst = bytearray(b"\xee" * q)
    plain = amd.LZ4HIPBatch.compress(src, so, [len(s) for s, _ in rs], plain_dst, do, [c for _, c in rs])
    outs = []
    for L in (0, 1, 7):
        with amd.LZ4Dictionary(b[:L]) as handle:
            got, dst, _ = host_batch(amd, handle, rs)
        outs.append((got, bytes(dst)))
        for i, (rec, c) in enumerate(rs):
            assert bytes(dst[do[i]:do[i] + got[i]]) == ref_compress(rd, b"", rec)[1], (L, i, len(rec))
    assert outs[0] == outs[1] == outs[2]
    got, dst = outs[0]
    for i in range(len(big)):
        assert got[i] == plain[i] and dst[do[i]:do[i] + got[i]] == bytes(plain_dst[do[i]:do[i] + plain[i]]), len(big[i])
    differ = sum(dst[do[i]:do[i] + got[i]] != bytes(plain_dst[do[i]:do[i] + plain[i]]) for i in range(len(big), len(rs)))
    assert differ >= 50, differ


def test_dictc_arguments_on_a_device(amd):
    l = amd.lib()
    src, dst = (C.c_uint8 * 32)(*range(32)), (C.c_uint8 * 64)()
    so, sl, do, dc, res = (C.c_uint64 * 1)(0), (C.c_int32 * 1)(32), (C.c_uint64 * 1)(0), (C.c_int32 * 1)(64), (C.c_int32 * 1)(7)
    assert l.lz4hip_compress_fast_dict_batch(src, so, sl, dst, do, dc, res, 1, None) == -3 and res[0] == 7
    assert l.lz4hip_compress_fast_dict_batch(src, so, sl, dst, do, dc, res, 0, None) == 0
    assert l.lz4hip_compress_fast_dict(src, 32, dst, 64, None) == -2 ** 31 + 3
    assert l.lz4hip_compress_fast_dict_batch_dev(src, so, sl, dst, do, dc, res, 1, None, 0, None) == -3
    with amd.LZ4Dictionary(b"0123456789") as h:
        assert l.lz4hip_compress_fast_dict_batch_dev(src, so, sl, dst, do, dc, res, 1, h._handle(), 99, None) == -3
        assert l.lz4hip_compress_fast_dict_batch_dev(None, so, sl, dst, do, dc, res, 1, h._handle(), 0, None) == -3
        # a negative length, a negative capacity: 0, like lz4hip_compress_fast
        sl2, dc2 = (C.c_int32 * 2)(-1, 32), (C.c_int32 * 2)(64, -1)
        so2, do2, res2 = (C.c_uint64 * 2)(0, 0), (C.c_uint64 * 2)(0, 0), (C.c_int32 * 2)(7, 7)
        assert l.lz4hip_compress_fast_dict_batch(src, so2, sl2, dst, do2, dc2, res2, 2, h._handle()) == 0 and list(res2) == [0, 0]
        assert bytes(dst) == bytes(64)
        # the same and a length above 0x7E000000 on device pointers (the host path would stage that many bytes; the kernel looks at
        # the length before it reads anything)
        import torch
        dev = torch.device("cuda", 0)
        t = lambda v, ty: torch.tensor(v, dtype=ty, device=dev)
        d_src, d_dst = torch.zeros(64, dtype=torch.uint8, device=dev), torch.full((128,), 0xEE, dtype=torch.uint8, device=dev)
        out = torch.full((3,), 7, dtype=torch.int32, device=dev)
        amd.DeviceBatch.compress_dict(d_src, t([0, 0, 0], torch.int64), t([-1, 32, 0x7E000001], torch.int32), d_dst, t([0, 0, 0], torch.int64),
                                      t([64, -1, 64], torch.int32), out, h)
        torch.cuda.synchronize()
        assert out.cpu().tolist() == [0, 0, 0] and bool((d_dst == 0xEE).all())


def test_dictc_cpp_mirror(tmp_path, rd):
    exe = build_mirror("dictc_mirror_test", tmp_path)
    b = book1()
    for L, n in ((100, 300), (65536, 4096), (4096, 0)):
        dp, sp, op = tmp_path / "d.bin", tmp_path / "s.bin", tmp_path / "o.bin"
        dp.write_bytes(b[:L]); sp.write_bytes(b[200000:200000 + n])
        p = subprocess.run([exe, str(dp), str(sp), str(op)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (L, n, p.stderr)
        wr, wb = ref_compress(rd, b[:L], b[200000:200000 + n])
        assert int(p.stdout.decode().strip()) == wr and op.read_bytes() == wb, (L, n)


def test_dictc_jni_shim(tmp_path, rd):
    exe = build_fake_jni("fake_jni_dictc", tmp_path)
    b = book1()
    for L, n in ((4096, 1000), (65537, 4096), (9, 300)):
        dp, sp = tmp_path / "d.bin", tmp_path / "s.bin"
        dp.write_bytes(b[:L]); sp.write_bytes(b[200000:200000 + n])
        out = subprocess.check_output([exe, str(dp), str(sp), str(tmp_path)], timeout=120).decode()
        assert "checks ok" in out, out
        assert (tmp_path / "dictc.bin").read_bytes() == ref_compress(rd, b[:L], b[200000:200000 + n])[1], (L, n)


def test_dictc_multidev_host_path():
    """lz4hip_init([0] * 2): the host batch takes the multi-device branch (block ranges per listed device, the handle's image on each)"""
    assert "dictc multidev ok D=2" in run_child("dictc_multidev_child.py", "2", timeout=300)
