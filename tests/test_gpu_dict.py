"""The dictionary decoder (LZ4_decompress_safe_usingDict, external dictionary) on the GPU against the reference library's own function:
the shared set of tests/dict_common.py (every stream x capacity x dictionary) in device batches of 3000 / 1 / 63 / 64 / 65 blocks with
guard bytes around every destination slot, both kernels (below and from 40960 blocks on), the host batch, coalesced single calls from
eight threads on two handles, a handle of length 0, the Python layers, the C++ mirror, the JNI shim and the multi-device host path."""
import ctypes as C
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from dict_common import DICT_LENS, RefDict, book1, caps_for, case_set, rng_for
from support import build_fake_jni, build_mirror, run_child

pytestmark = pytest.mark.gpu
GUARD = 8
BIG_CAP_STREAM = 1200   # the capacity 255 * stream + 64 of the list is kept for streams up to this size (device memory and time)


@pytest.fixture(scope="module")
def rd(ref):
    return RefDict(ref)


@pytest.fixture(scope="module")
def rows(rd):
    """{L: [(stream, cap)]} over the whole shared set, and the reference's (value, bytes) for each row, computed once"""
    _, cases = case_set(rd, rng_for(11))
    b = book1()
    by_len = {L: [] for L in DICT_LENS}
    for name, s, d, L in cases:
        for cap in caps_for(d, len(s)):
            if cap > d + 607 and len(s) > BIG_CAP_STREAM:
                continue
            by_len[L].append((s, cap))
    want = {L: [rd.decode(s, cap, b[:L]) for s, cap in r] for L, r in by_len.items()}
    assert sum(len(r) for r in by_len.values()) > 30000
    return by_len, want


def layout(rs):
    """one source buffer, one destination buffer with GUARD bytes in front of, between and behind the slots"""
    so, do, p, q = [], [], 0, GUARD
    for s, c in rs:
        so.append(p); do.append(q); p += len(s); q += c + GUARD
    return b"".join(s for s, _ in rs) + b"\0", so, do, q


def check(rs, want, got, dst, do, what, exact_tail):
    """values, bytes, and 0xEE everywhere outside the slots (exact_tail: behind the decoded bytes too -- the host path hands back
    exactly those)"""
    dst = bytes(dst)
    assert dst[:GUARD] == b"\xee" * GUARD, (what, "written in front of the first slot")
    for i, ((s, c), (r, by)) in enumerate(zip(rs, want)):
        assert int(got[i]) == r, (what, i, len(s), c, int(got[i]), r)
        o = do[i]
        assert dst[o:o + max(r, 0)] == by, (what, "bytes", i, len(s), c)
        tail = dst[o + (max(r, 0) if exact_tail else c):o + c + GUARD]
        assert tail == b"\xee" * len(tail), (what, "written outside the slot", i, len(s), c)


def device_batch(amd, rs, dict_t, dev):
    import torch
    src, so, do, q = layout(rs)
    d_src = torch.frombuffer(bytearray(src), dtype=torch.uint8).to(dev)
    d_dst = torch.full((q,), 0xEE, dtype=torch.uint8, device=dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    out = torch.full((len(rs),), -12345, dtype=torch.int32, device=dev)
    amd.DeviceBatch.decompress_safe_dict(d_src, i64(so), i32([len(s) for s, _ in rs]), d_dst, i64(do), i32([c for _, c in rs]), out, dict_t)
    torch.cuda.synchronize()
    return out.cpu().tolist(), d_dst.cpu().numpy().tobytes(), do


@pytest.mark.parametrize("L", DICT_LENS)
def test_dict_device_batches(amd, rows, L):
    """the set of one dictionary in device batches of 3000 blocks, and batches of 1 / 63 / 64 / 65 out of it"""
    import torch
    by_len, want = rows
    rs, w = by_len[L], want[L]
    dev = torch.device("cuda", 0)
    dict_t = torch.frombuffer(bytearray(book1()[:L]), dtype=torch.uint8).to(dev)
    chunks = [(k, min(k + 3000, len(rs))) for k in range(0, len(rs), 3000)]
    rng = rng_for(L)
    for size in (1, 63, 64, 65):
        k = rng.randrange(0, len(rs) - size)
        chunks.append((k, k + size))
    for a, e in chunks:
        got, dst, do = device_batch(amd, rs[a:e], dict_t, dev)
        check(rs[a:e], w[a:e], got, dst, do, "device batch %d:%d of L=%d" % (a, e, L), exact_tail=False)


@pytest.mark.parametrize("L", (100, 65536))
def test_dict_both_kernels(amd, rd, L):
    """40959 blocks (decode_dict_deep_kernel) and 40960 (decode_dict_kernel): short records, valid, damaged and cut, side by side in
    the wavefronts; guard bytes around every slot"""
    import torch
    b = book1()
    d = b[:L]
    rng = rng_for(40 + L)
    base = []
    for k in range(24):
        size = (300, 1000, 2000)[k % 3]
        o = rng.randrange(200000, len(b) - size)
        s = rd.compress(d, b[o:o + size], 9 if k % 2 else 0)
        if k % 6 == 4:
            s = s[:rng.randrange(len(s))]
        if k % 6 == 5:
            s = bytes(x if rng.random() > 0.01 else rng.randrange(256) for x in s)
        base.append(s)
    slot = 2000
    caps = (2000, 1999, 300, 1000, 999, 64)
    cache = {}
    dev = torch.device("cuda", 0)
    dict_t = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev)
    src = b"".join(base) + b"\0"
    boff = np.concatenate([[0], np.cumsum([len(s) for s in base])[:-1]])
    d_src = torch.frombuffer(bytearray(src), dtype=torch.uint8).to(dev)
    for n in (40959, 40960):
        idx = np.array([rng.randrange(len(base)) for _ in range(n)])
        cp = np.array([caps[rng.randrange(len(caps))] for _ in range(n)], dtype=np.int32)
        so = torch.tensor(boff[idx], dtype=torch.int64, device=dev)
        sl = torch.tensor(np.array([len(base[k]) for k in idx], dtype=np.int32), device=dev)
        do = np.arange(n, dtype=np.int64) * (slot + GUARD) + GUARD
        d_dst = torch.full((n * (slot + GUARD) + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
        out = torch.full((n,), -12345, dtype=torch.int32, device=dev)
        amd.DeviceBatch.decompress_safe_dict(d_src, so, sl, d_dst, torch.tensor(do, device=dev), torch.tensor(cp, device=dev), out, dict_t)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        dst = d_dst.cpu().numpy()
        assert (dst[:GUARD] == 0xEE).all()
        rows2 = dst[GUARD:].reshape(n, slot + GUARD)
        for k in range(len(base)):
            for c in caps:
                sel = np.nonzero((idx == k) & (cp == c))[0]
                if not len(sel):
                    continue
                if (k, c) not in cache:
                    cache[(k, c)] = rd.decode(base[k], c, d)
                r, by = cache[(k, c)]
                assert (got[sel] == r).all(), (n, k, c, r, got[sel][:5])
                assert (rows2[sel, :max(r, 0)] == np.frombuffer(by, dtype=np.uint8)).all(), (n, k, c, "bytes")
                assert (rows2[sel, c:] == 0xEE).all(), (n, k, c, "written outside the slot")


def test_dict_host_batch(amd, rows):
    """the host batch (LZ4HIPBatch.decompressSafeDict on a handle): every third row of three dictionaries; exactly the decoded bytes
    come back"""
    by_len, want = rows
    b = book1()
    for L in (3, 4096, 100000):
        rs, w = by_len[L][::3], want[L][::3]
        with amd.LZ4Dictionary(b[:L]) as handle:
            assert len(handle) == L
            src, so, do, q = layout(rs)
            dst = bytearray(b"\xee" * q)
            got = amd.LZ4HIPBatch.decompressSafeDict(src, so, [len(s) for s, _ in rs], dst, do, [c for _, c in rs], handle)
        check(rs, w, got, dst, do, "host batch L=%d" % L, exact_tail=True)


def test_dict_single_calls_from_eight_threads_on_two_handles(amd, rows):
    """single calls coalesce per handle: eight threads alternate between two dictionaries, every call gets its own dictionary's answer"""
    by_len, want = rows
    b = book1()
    La, Lb = 4096, 65537
    ha, hb = amd.LZ4Dictionary(b[:La]), amd.LZ4Dictionary(b[:Lb])
    d = amd.LZ4Factory.hipInstance().safeDecompressor()
    jobs = [(La, ha, i) for i in range(0, len(by_len[La]), 41)] + [(Lb, hb, i) for i in range(0, len(by_len[Lb]), 41)]
    jobs = [j for pair in zip(jobs[:len(jobs) // 2], jobs[len(jobs) // 2:]) for j in pair]   # (the two handles interleaved)

    def one(job):
        L, h, i = job
        s, c = by_len[L][i]
        buf = bytearray(b"\xee" * (c + GUARD + 3))
        try:
            r = d.decompressWithDict(h, s, 0, len(s), buf, 3, c)
        except amd.LZ4Exception as e:
            return ("error", str(e)), buf
        return r, buf

    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, jobs))
    assert len(jobs) > 200
    for (L, h, i), (r, buf) in zip(jobs, res):
        s, c = by_len[L][i]
        wr, wb = want[L][i]
        if wr < 0:
            assert r == ("error", "Error decoding offset %d of input buffer" % (-wr)), (L, i, r, wr)
            assert bytes(buf[3 + c:]) == b"\xee" * GUARD
        else:
            assert r == wr and bytes(buf[3:3 + r]) == wb, (L, i, len(s), c, r, wr)
            assert bytes(buf[3 + r:]) == b"\xee" * (len(buf) - 3 - r)
        assert buf[:3] == b"\xee\xee\xee"
    ha.close(); hb.close()


def test_dict_handle_of_length_0_is_the_safe_decoder(amd, ref, rd, rows):
    """dict_len == 0 (handle and device pointer): the values and bytes of lz4hip_decompress_safe* and of the reference's plain decoder"""
    import torch
    by_len, _ = rows
    b = book1()
    rs = [(ref.compress_fast(b[k * 5000:k * 5000 + 4000]), c) for k in range(6) for c in (3999, 4000, 4100)] + by_len[4096][:600:3]
    src, so, do, q = layout(rs)
    sl, cp = [len(s) for s, _ in rs], [c for _, c in rs]
    plain_dst = bytearray(b"\xee" * q)
    plain = amd.LZ4HIPBatch.decompressSafe(src, so, sl, plain_dst, do, cp)
    assert plain == [rd.plain(s, c) for s, c in rs]
    with amd.LZ4Dictionary(b"") as h0:
        assert len(h0) == 0
        dst = bytearray(b"\xee" * q)
        assert amd.LZ4HIPBatch.decompressSafeDict(src, so, sl, dst, do, cp, h0) == plain
        assert dst == plain_dst
        buf = bytearray(5000)
        assert amd.LZ4SafeDecompressor().decompressWithDict(h0, rs[1][0], 0, len(rs[1][0]), buf, 0, 4000) == 4000 and bytes(buf[:4000]) == b[:4000]
    dev = torch.device("cuda", 0)
    got, ddst, _ = device_batch(amd, rs, torch.empty(0, dtype=torch.uint8, device=dev), dev)
    assert got == plain
    check(rs, [(r, bytes(plain_dst[o:o + max(r, 0)])) for r, o in zip(plain, do)], got, ddst, do, "device, no dictionary", exact_tail=False)


def test_dict_python_layers_and_arguments(amd, rd):
    """LZ4Dictionary: length, context manager, use after close; the C ABI's argument errors on a device; the device entry point takes
    the whole dictionary or its last 64 KB alike"""
    import torch
    l = amd.lib()
    b = book1()
    h = amd.LZ4Dictionary(bytearray(b[:70000]))
    assert len(h) == 70000 and "70000" in repr(h)
    h.close(); h.close()
    with pytest.raises(AssertionError):
        len(h)
    with pytest.raises(AssertionError):
        amd.LZ4SafeDecompressor().decompressWithDict(h, b"\x10a", 0, 2, bytearray(8), 0)
    out = C.c_void_p(None)
    assert l.lz4hip_dict_create(None, 4, C.byref(out)) == -3 and l.lz4hip_dict_create(b"abcd", -1, C.byref(out)) == -3
    assert l.lz4hip_dict_create(b"abcd", 4, None) == -3 and not out
    assert l.lz4hip_dict_size(None) == -3
    l.lz4hip_dict_free(None)
    src, dst = (C.c_uint8 * 8)(0x10, 0x61), (C.c_uint8 * 8)()
    so, sl, do, dc, res = (C.c_uint64 * 1)(0), (C.c_int32 * 1)(2), (C.c_uint64 * 1)(0), (C.c_int32 * 1)(8), (C.c_int32 * 1)(7)
    assert l.lz4hip_decompress_safe_dict_batch(src, so, sl, dst, do, dc, res, 1, None) == -3 and res[0] == 7
    assert l.lz4hip_decompress_safe_dict_batch(src, so, sl, dst, do, dc, res, 0, None) == 0
    assert l.lz4hip_decompress_safe_dict(src, 2, dst, 8, None) == -2 ** 31 + 3
    assert l.lz4hip_decompress_safe_dict_batch_dev(src, so, sl, dst, do, dc, res, 1, None, 5, 0, None) == -3
    assert l.lz4hip_decompress_safe_dict_batch_dev(src, so, sl, dst, do, dc, res, 1, src, -1, 0, None) == -3
    assert l.lz4hip_decompress_safe_dict_batch_dev(src, so, sl, dst, do, dc, res, 1, src, 4, 99, None) == -3
    # the whole 100000-byte dictionary and its last 65536 bytes reach the same bytes
    dev = torch.device("cuda", 0)
    d = b[:100000]
    rs = []
    rng = rng_for(77)
    for _ in range(40):
        o = rng.randrange(200000, len(b) - 4096)
        rs.append((rd.compress(d, b[o:o + 4096], 9), 4096))
    want = [rd.decode(s, c, d) for s, c in rs]
    assert all(r == 4096 for r, _ in want)
    for t in (d, d[-65536:], d[-70000:]):
        got, dst2, do2 = device_batch(amd, rs, torch.frombuffer(bytearray(t), dtype=torch.uint8).to(dev), dev)
        check(rs, want, got, dst2, do2, "dictionary tail of %d bytes" % len(t), exact_tail=False)


def _pick(rows, L, count):
    by_len, want = rows
    rs, w = by_len[L], want[L]
    step = max(1, len(rs) // count)
    return [(rs[i], w[i]) for i in range(0, len(rs), step) if len(rs[i][0]) > 0]


def test_dict_cpp_mirror(tmp_path, rows):
    exe = build_mirror("dict_mirror_test", tmp_path)
    b = book1()
    for L in (100, 65536):
        dp = tmp_path / ("d%d.bin" % L)
        dp.write_bytes(b[:L])
        for (s, c), (wr, wb) in _pick(rows, L, 10):
            sp, op = tmp_path / "s.bin", tmp_path / "o.bin"
            sp.write_bytes(s)
            p = subprocess.run([exe, str(dp), str(sp), str(c), str(op)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            assert p.returncode == 0, (L, len(s), c, p.stderr)
            line = p.stdout.decode().strip()
            if wr < 0:
                assert line == "error Error decoding offset %d of input buffer" % (3 - wr), (L, line, wr)
            else:
                assert int(line) == wr and op.read_bytes() == wb, (L, line, wr)


def test_dict_jni_shim(tmp_path, rows):
    exe = build_fake_jni("fake_jni_dict", tmp_path)
    b = book1()
    for L in (4096, 65537):
        dp = tmp_path / ("d%d.bin" % L)
        dp.write_bytes(b[:L])
        for (s, c), (wr, wb) in _pick(rows, L, 8):
            sp = tmp_path / "s.bin"
            sp.write_bytes(s)
            out = subprocess.check_output([exe, str(dp), str(sp), str(c), str(tmp_path)], timeout=120).decode()
            assert "checks ok" in out, out
            assert int((tmp_path / "dict.txt").read_text()) == wr, (L, len(s), c, wr)
            if wr > 0:
                assert (tmp_path / "dict.bin").read_bytes() == wb, (L, len(s), c)


def test_dict_multidev_host_path():
    """lz4hip_init([0] * 2): the host batch takes the multi-device branch (block ranges per listed device, the handle on each)"""
    assert "dict multidev ok D=2" in run_child("dict_multidev_child.py", "2", timeout=600)
