"""The dictionary HC compressor (LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream, external dictionary) on the GPU against
the reference library's own functions: the shared set of tests/hcdict_common.py through the host batch, per dictionary and level; the
repeated-pattern and hand-built cases against their own dictionaries; device batches with guard bytes round every slot, in two fills,
with slots of exactly the five capacities, with the caller's workspace and with a span one byte short; mixed lengths in one launch; round
trips through the dictionary decoder; one handle used by the fast and the HC compressor; coalesced single calls from eight threads on
two handles and two levels; the first-use image build raced by two streams; the C++ mirror, the JNI shim and two devices.  Every size a
test states to the host path is true of the buffer it passes; malformed sizes go to device pointers with guarded slots only."""
import ctypes as C
import subprocess
import threading
from concurrent.futures import ThreadPoolExecutor

import pytest

from hcdict_common import (BIG_LEVELS, BIG_SIZES, CLAMPS, DICT_LENS, LEVELS, SMALL_SIZES, Ref, book1, book_records, bound, caps_for, clamp,
                           dict_cuts, hand_cases, has_dict_match, other_records, parse, pattern_cases)
from support import build_fake_jni, build_mirror, run_child

pytestmark = pytest.mark.gpu
GUARD = 8


@pytest.fixture(scope="module")
def R(ref):
    return Ref(ref)


def rows_for(R, d, recs, level, all_caps=True):
    """[(record, capacity)] and the reference's (value, bytes) per row: the bound, the exact size, one byte less, 1 and 0"""
    rs, want = [], []
    for name, rec in recs:
        full = R.compress(d, rec, level)
        for cap in (caps_for(len(rec), full[0], True) if all_caps else [bound(len(rec))]):
            rs.append((rec, cap))
            want.append(full if cap >= full[0] else R.compress(d, rec, level, cap))
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


def host_batch(amd, handle, rs, level):
    src, so, do, q = layout(rs)
    dst = bytearray(b"\xee" * q)
    got = amd.LZ4HIPBatch.compressHCDict(src, so, [len(s) for s, _ in rs], dst, do, [c for _, c in rs], handle, level)
    return got, dst, do


@pytest.mark.parametrize("L", DICT_LENS)
def test_hcdict_host_batches(amd, R, L):
    """book1[:L] through the host batch: the small book records at the five capacities and the 200 pattern records, one batch per
    level and clamp; the big book records and the records cut out of the dictionary at level 9 and one optimal level"""
    d = book1()[:L]
    small = book_records(SMALL_SIZES)
    pats = [(name, rec) for name, _, rec in pattern_cases()]
    big = book_records(BIG_SIZES) + dict_cuts(L, __import__("random").Random(300 + L))
    with amd.LZ4Dictionary(d) as handle:
        for level in LEVELS + tuple(a for a, _ in CLAMPS):
            rs, want = rows_for(R, d, small, clamp(level))
            r2, w2 = rows_for(R, d, pats, clamp(level), all_caps=False)
            got, dst, do = host_batch(amd, handle, rs + r2, level)
            check(rs + r2, want + w2, got, dst, do, "host batch, L=%d level %d" % (L, level), exact_tail=True)
        for level in BIG_LEVELS:
            rs, want = rows_for(R, d, big, level, all_caps=False)
            got, dst, do = host_batch(amd, handle, rs, level)
            check(rs, want, got, dst, do, "big host batch, L=%d level %d" % (L, level), exact_tail=True)


@pytest.mark.parametrize("part", range(4))
def test_hcdict_pattern_cases_against_their_dictionaries(amd, R, part):
    """50 of the 200 repeated-pattern cases, each against its own dictionary, at every level"""
    for name, d, rec in pattern_cases()[part * 50:(part + 1) * 50]:
        with amd.LZ4Dictionary(d) as handle:
            for level in LEVELS:
                rs, want = rows_for(R, d, [(name, rec)], level, all_caps=False)
                got, dst, do = host_batch(amd, handle, rs, level)
                check(rs, want, got, dst, do, "%s level %d" % (name, level), exact_tail=True)


def test_hcdict_hand_built_cases(amd, R):
    """the hand-built cases: the reference's level 9 output holds the intended sequence, and the engine's bytes are the reference's at
    every capacity and level"""
    for name, d, rec, chk in hand_cases():
        chk(parse(R.compress(d, rec, 9)[1]))
        with amd.LZ4Dictionary(d) as handle:
            for level in (LEVELS if len(rec) <= 4096 else BIG_LEVELS):
                rs, want = rows_for(R, d, [(name, rec)], level)
                got, dst, do = host_batch(amd, handle, rs, level)
                check(rs, want, got, dst, do, "%s level %d" % (name, level), exact_tail=True)


def dev_tensors(torch, recs, caps, G, fill):
    so, do, p, q = [], [], 0, G
    for rec, c in zip(recs, caps):
        so.append(p); do.append(q); p += len(rec); q += c + G
    dev = torch.device("cuda", 0)
    d_src = torch.frombuffer(bytearray(b"".join(recs) + b"\0"), dtype=torch.uint8).to(dev)
    d_dst = torch.full((q,), fill, dtype=torch.uint8, device=dev)
    t = lambda v, ty: torch.tensor(v, dtype=ty, device=dev)
    return d_src, t(so, torch.int64), t([len(r) for r in recs], torch.int32), d_dst, t(do, torch.int64), t(caps, torch.int32), so, do


def test_hcdict_device_batch_guards_two_fills_five_capacities(amd, R):
    """one device batch per level (9 and 10): every record at exactly the five capacities, 64 guard bytes in front of and behind every
    slot; a second run with another fill gives the same values and bytes, and the guards of both are untouched"""
    import torch
    G = 64
    d = book1()[:65536]
    recs0 = [rec for _, rec in book_records(SMALL_SIZES + BIG_SIZES[:1]) + dict_cuts(65536, __import__("random").Random(17))]
    with amd.LZ4Dictionary(d) as handle:
        for level in (9, 10):
            recs, caps, want = [], [], []
            for rec in recs0:
                full = R.compress(d, rec, level)
                for cap in caps_for(len(rec), full[0], True):
                    recs.append(rec); caps.append(cap)
                    want.append(full if cap >= full[0] else R.compress(d, rec, level, cap))
            runs = []
            for fill in (0xEE, 0x11):
                d_src, so, sl, d_dst, do, dc, _, dof = dev_tensors(torch, recs, caps, G, fill)
                out = torch.full((len(recs),), -12345, dtype=torch.int32, device=d_src.device)
                amd.DeviceBatch.compress_hc_dict_sync(d_src, so, sl, d_dst, do, dc, out, handle, level)
                torch.cuda.synchronize()
                got, dst = out.cpu().tolist(), d_dst.cpu().numpy().tobytes()
                assert dst[:G] == bytes([fill]) * G
                for i, (r, by) in enumerate(want):
                    assert got[i] == r, (level, i, len(recs[i]), caps[i], got[i], r)
                    assert dst[dof[i]:dof[i] + r] == by, ("bytes", level, i, len(recs[i]))
                    assert dst[dof[i] + caps[i]:dof[i] + caps[i] + G] == bytes([fill]) * G, ("guard behind slot", level, i, caps[i])
                runs.append((got, [dst[dof[i]:dof[i] + max(got[i], 0)] for i in range(len(recs))]))
            assert runs[0] == runs[1]


def test_hcdict_caller_workspace_exact_and_one_byte_short(amd, R):
    """the _ws form: with a workspace of exactly lz4hip_hc_workspace_bytes the results are the reference's and the bytes behind the
    workspace do not change; with a span one byte short the block that reaches the span's end gives 0, the others are unchanged, and
    nothing is written past the (smaller) workspace"""
    import torch
    b = book1()
    d = b[:4096]
    recs = [b[200000 + 5000 * i:200000 + 5000 * i + n] for i, n in enumerate((1000, 13, 4096, 300, 2000))]
    caps = [bound(len(r)) for r in recs]
    span = sum(len(r) for r in recs)
    with amd.LZ4Dictionary(d) as handle:
        for level in (9, 10):
            want = [R.compress(d, rec, level) for rec in recs]
            for short in (0, 1):
                d_src, so, sl, d_dst, do, dc, _, dof = dev_tensors(torch, recs, caps, GUARD, 0xEE)
                nb = amd.lib().lz4hip_hc_workspace_bytes(span - short, len(recs), level)
                ws = torch.full((nb + 4096,), 0x77, dtype=torch.uint8, device=d_src.device)
                out = torch.full((len(recs),), -12345, dtype=torch.int32, device=d_src.device)
                amd.DeviceBatch.compress_hc_dict(d_src, so, sl, d_dst, do, dc, out, handle, level, span=span - short, ws=ws[:nb])
                torch.cuda.synchronize()
                got, dst = out.cpu().tolist(), d_dst.cpu().numpy().tobytes()
                assert bool((ws[nb:] == 0x77).all()), ("written past the workspace", level, short)
                for i, (r, by) in enumerate(want):
                    if short and i == len(recs) - 1:
                        assert got[i] == 0 and dst[dof[i]:dof[i] + caps[i]] == b"\xee" * caps[i], (level, got[i])
                    else:
                        assert got[i] == r and dst[dof[i]:dof[i] + r] == by, (level, short, i, got[i], r)
            # a workspace one byte too small for the span it is said to be for is an argument error
            assert amd.lib().lz4hip_compress_hc_dict_batch_dev_ws(d_src.data_ptr(), so.data_ptr(), sl.data_ptr(), d_dst.data_ptr(), do.data_ptr(),
                                                                  dc.data_ptr(), out.data_ptr(), len(recs), level, handle._handle(), 0, None,
                                                                  span, ws.data_ptr(), amd.lib().lz4hip_hc_workspace_bytes(span, len(recs), level) - 1) == -3


def test_hcdict_mixed_lengths_in_one_launch(amd, R, O, corpus):
    """lengths 0 .. 70000 in one launch, one launch each at levels 9 and 10"""
    import torch
    d = book1()[:65537]
    recs = [rec for _, rec in book_records(SMALL_SIZES + BIG_SIZES[:1]) + other_records(O, corpus, n_rnd=24)]
    assert min(len(r) for r in recs) == 0 and max(len(r) for r in recs) == 70000
    caps = [bound(len(r)) for r in recs]
    with amd.LZ4Dictionary(d) as handle:
        for level in (9, 10):
            want = [R.compress(d, rec, level) for rec in recs]
            d_src, so, sl, d_dst, do, dc, _, dof = dev_tensors(torch, recs, caps, GUARD, 0xEE)
            out = torch.full((len(recs),), -12345, dtype=torch.int32, device=d_src.device)
            amd.DeviceBatch.compress_hc_dict(d_src, so, sl, d_dst, do, dc, out, handle, level)
            torch.cuda.synchronize()
            got, dst = out.cpu().tolist(), d_dst.cpu().numpy().tobytes()
            for i, (r, by) in enumerate(want):
                assert got[i] == r and dst[dof[i]:dof[i] + r] == by, (level, i, len(recs[i]), got[i], r)
                assert dst[dof[i] + caps[i]:dof[i] + caps[i] + GUARD] == b"\xee" * GUARD


def test_hcdict_round_trips(amd, R):
    """records compressed here decode back to the input through lz4hip_decompress_safe_dict_batch; most of them reach into the
    dictionary"""
    import random
    b = book1()
    rng = random.Random(19)
    for L, level in ((4, 9), (4096, 1), (65536, 9), (100000, 10)):
        d = b[:L]
        recs = []
        for _ in range(100):
            n = rng.choice([13, 64, 300, 1000, 4096])
            o = rng.randrange(200000, len(b) - n)
            recs.append(b[o:o + n])
        recs += [x for _, x in dict_cuts(L, rng)]
        rs = [(rec, bound(len(rec))) for rec in recs]
        with amd.LZ4Dictionary(d) as handle:
            got, dst, do = host_batch(amd, handle, rs, level)
            streams = [bytes(dst[o:o + r]) for o, r in zip(do, got)]
            assert all(r > 0 for r in got)
            back_rs = [(s, len(rec)) for s, rec in zip(streams, recs)]
            src, so, do2, q = layout(back_rs)
            back = bytearray(b"\xee" * q)
            r2 = amd.LZ4HIPBatch.decompressSafeDict(src, so, [len(s) for s in streams], back, do2, [len(rec) for rec in recs], handle)
        for i, rec in enumerate(recs):
            assert r2[i] == len(rec) and bytes(back[do2[i]:do2[i] + len(rec)]) == rec, (L, i, len(rec))
        if L >= 4096:
            uses = sum(has_dict_match(parse(s)) for s, rec in zip(streams, recs) if len(rec) >= 300)
            assert uses >= 0.9 * sum(len(rec) >= 300 for rec in recs), (L, uses)


def test_hcdict_one_handle_for_the_fast_and_the_hc_compressor(amd, R, ref):
    """the same handle used by lz4hip_compress_fast_dict first and by the HC compressor after, then by the fast one again: the two
    images coexist"""
    from dictc_common import ref_compress
    from dict_common import RefDict
    rd = RefDict(ref)
    b = book1()
    d, rec = b[:65536], b[200000:204096]
    fast, hc = amd.LZ4HIPCompressor(), amd.LZ4HCHIPCompressor(9)
    with amd.LZ4Dictionary(d) as handle:
        for _ in range(2):
            assert fast.compressWithDict(handle, rec) == ref_compress(rd, d, rec)[1]
            assert hc.compressWithDict(handle, rec) == R.compress(d, rec, 9)[1]
        assert amd.LZ4HCHIPCompressor(3).compressWithDict(handle, rec) == R.compress(d, rec, 3)[1]


def test_hcdict_single_calls_from_eight_threads_on_two_handles_and_two_levels(amd, R):
    """single calls coalesce per handle and clamped level: eight threads alternate between two dictionaries and two levels, every call
    gets its own dictionary's bytes at its own level"""
    import random
    b = book1()
    rng = random.Random(18)
    da, db = b[:4096], b[:65537]
    recs = []
    for _ in range(40):
        n = rng.choice([0, 12, 13, 64, 300, 1000, 4096])
        o = rng.randrange(200000, len(b) - n)
        recs.append(b[o:o + n])
    jobs = [(d, h, lv, rec) for rec in recs for d, h in ((da, 0), (db, 1)) for lv in (4, 9)]
    want = [R.compress(d, rec, lv) for d, h, lv, rec in jobs]
    handles = [amd.LZ4Dictionary(da), amd.LZ4Dictionary(db)]
    comp = {lv: amd.LZ4HCHIPCompressor(lv) for lv in (4, 9)}

    def one(job):
        d, h, lv, rec = job
        buf = bytearray(b"\xee" * (bound(len(rec)) + GUARD + 3))
        r = comp[lv].compressWithDict(handles[h], rec, 0, len(rec), buf, 3, bound(len(rec)))
        return r, buf

    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, jobs))
    assert len(jobs) == 160
    for (d, h, lv, rec), (r, buf), (wr, wb) in zip(jobs, res, want):
        assert r == wr and bytes(buf[3:3 + r]) == wb, (len(d), lv, len(rec), r, wr)
        assert bytes(buf[3 + r:]) == b"\xee" * (len(buf) - 3 - r) and buf[:3] == b"\xee\xee\xee"
    # a capacity one byte short is the HC compressor's exception (no message), and writes nothing past the slot
    rec = recs[5]
    wr = R.compress(da, rec, 9)[0]
    buf = bytearray(b"\xee" * (wr + GUARD))
    with pytest.raises(amd.LZ4Exception):
        comp[9].compressWithDict(handles[0], rec, 0, len(rec), buf, 0, wr - 1)
    assert bytes(buf[wr - 1:]) == b"\xee" * (GUARD + 1)
    for h in handles:
        h.close()


def test_hcdict_first_use_image_build_raced_by_two_streams(amd, R):
    """two threads, each on a stream of its own, make a fresh handle's first HC compress at the same time: one builds the image, both
    get the reference's bytes"""
    import torch
    b = book1()
    d = b[:65536]
    recs = [b[200000 + 3000 * i:200000 + 3000 * i + 2500] for i in range(16)]
    caps = [bound(len(r)) for r in recs]
    want = [R.compress(d, rec, 9) for rec in recs]
    for attempt in range(3):
        handle = amd.LZ4Dictionary(d)
        start = threading.Barrier(2)
        res = [None, None]

        def work(k):
            st = torch.cuda.Stream(device=0)
            with torch.cuda.stream(st):
                d_src, so, sl, d_dst, do, dc, _, dof = dev_tensors(torch, recs, caps, GUARD, 0xEE)
                out = torch.full((len(recs),), -12345, dtype=torch.int32, device=d_src.device)
                st.synchronize()
                start.wait()
                amd.DeviceBatch.compress_hc_dict(d_src, so, sl, d_dst, do, dc, out, handle, 9)
                st.synchronize()
                res[k] = (out.cpu().tolist(), d_dst.cpu().numpy().tobytes(), dof)

        ts = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for got, dst, dof in res:
            for i, (r, by) in enumerate(want):
                assert got[i] == r and dst[dof[i]:dof[i] + r] == by, (attempt, i, got[i], r)
        handle.close()


def test_hcdict_arguments_on_a_device(amd):
    l = amd.lib()
    src, dst = (C.c_uint8 * 32)(*range(32)), (C.c_uint8 * 64)()
    so, sl, do, dc, res = (C.c_uint64 * 1)(0), (C.c_int32 * 1)(32), (C.c_uint64 * 1)(0), (C.c_int32 * 1)(64), (C.c_int32 * 1)(7)
    assert l.lz4hip_compress_hc_dict_batch(src, so, sl, dst, do, dc, res, 1, 9, None) == -3 and res[0] == 7
    assert l.lz4hip_compress_hc_dict_batch(src, so, sl, dst, do, dc, res, 0, 9, None) == 0
    assert l.lz4hip_compress_hc_dict(src, 32, dst, 64, 9, None) == -2 ** 31 + 3
    assert l.lz4hip_compress_hc_dict_batch_dev(src, so, sl, dst, do, dc, res, 1, 9, None, 0, None) == -3
    with amd.LZ4Dictionary(b"0123456789") as h:
        assert l.lz4hip_compress_hc_dict_batch_dev(src, so, sl, dst, do, dc, res, 1, 9, h._handle(), 99, None) == -3
        assert l.lz4hip_compress_hc_dict_batch_dev(None, so, sl, dst, do, dc, res, 1, 9, h._handle(), 0, None) == -3
        assert l.lz4hip_compress_hc_dict_batch_dev_ws(src, so, sl, dst, do, dc, res, 1, 9, h._handle(), 0, None, 32, None, 0) == -3
        # a negative length, a negative capacity, a length above 0x7E000000: 0 -- on device pointers with guarded slots (the host
        # path stages what it is told; the kernels look at the sizes before they read anything)
        import torch
        dev = torch.device("cuda", 0)
        t = lambda v, ty: torch.tensor(v, dtype=ty, device=dev)
        d_src, d_dst = torch.zeros(64, dtype=torch.uint8, device=dev), torch.full((256,), 0xEE, dtype=torch.uint8, device=dev)
        for level in (9, 10):
            out = torch.full((3,), 7, dtype=torch.int32, device=dev)
            amd.DeviceBatch.compress_hc_dict(d_src, t([0, 0, 0], torch.int64), t([-1, 32, 0x7E000001], torch.int32), d_dst,
                                             t([64, 64, 64], torch.int64), t([64, -1, 64], torch.int32), out, h, level)
            torch.cuda.synchronize()
            assert out.cpu().tolist() == [0, 0, 0] and bool((d_dst == 0xEE).all())


def test_hcdict_cpp_mirror(tmp_path, R):
    exe = build_mirror("hcdict_mirror_test", tmp_path)
    b = book1()
    for L, n, level in ((100, 300, 9), (65536, 4096, 4), (4096, 0, 10)):
        dp, sp, op = tmp_path / "d.bin", tmp_path / "s.bin", tmp_path / "o.bin"
        dp.write_bytes(b[:L]); sp.write_bytes(b[200000:200000 + n])
        p = subprocess.run([exe, str(dp), str(sp), str(op), str(level)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (L, n, p.stderr)
        wr, wb = R.compress(b[:L], b[200000:200000 + n], level)
        assert int(p.stdout.decode().strip()) == wr and op.read_bytes() == wb, (L, n)


def test_hcdict_jni_shim(tmp_path, R):
    exe = build_fake_jni("fake_jni_hcdict", tmp_path)
    b = book1()
    for L, n, level in ((4096, 1000, 9), (65537, 4096, 3), (4, 300, 12)):
        dp, sp = tmp_path / "d.bin", tmp_path / "s.bin"
        dp.write_bytes(b[:L]); sp.write_bytes(b[200000:200000 + n])
        out = subprocess.check_output([exe, str(dp), str(sp), str(tmp_path), str(level)], timeout=120).decode()
        assert "checks ok" in out, out
        assert (tmp_path / "hcdict.bin").read_bytes() == R.compress(b[:L], b[200000:200000 + n], level)[1], (L, n)


def test_hcdict_two_devices():
    """lz4hip_init([0, 1]): the host batch shards over two devices, the handle's tail and HC image on each"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    assert "hcdict multidev ok D=2" in run_child("hcdict_multidev_child.py", "0", "1", timeout=300)
