"""The partial decoder (LZ4_decompress_safe_partial) on the GPU against the reference library's own LZ4_decompress_safe_partial: the
host batch, the device batch and coalesced single calls; the Python factory, LZ4HIPBatch, DeviceBatch, the C++ mirror and the JNI shim;
the multi-device host path; both kernels (below and from 40960 blocks on) with ragged targets side by side; guard bytes behind
min(target, cap) in every slot; the negative-size rule; the long-literal stream whose run liblz4 cuts."""
import ctypes as C
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import calgary
from partial_common import (caps_for, damaged, long_literal_stream, overlap_stream, ref_partial, rng_for, same_bytes,
                            targets_for)
from support import build_fake_jni, build_mirror, run_child

pytestmark = pytest.mark.gpu
GUARD = 8


@pytest.fixture(scope="module")
def lz4p(ref):
    return ref_partial(ref)


@pytest.fixture(scope="module")
def cases(ref, O):
    """[(stream, target, cap)]: valid streams of the Calgary corpus, App. F and book1 slices (LZ4_compress_default and HC level 12)
    at every target class and capacity class, cut streams, cuts inside self-overlapping matches, damaged and random streams"""
    rng = rng_for(21)
    book1, geo, pic = calgary("book1"), calgary("geo"), calgary("pic")
    raw = [book1[:65536], book1[400000:465536], geo[:65536], pic[:65536], O.gen_block(65536, 11), O.gen_block(65536, 12, win=8),
           O.gen_block(300000, 13), book1[:3000]]
    streams = []
    for v in raw:
        streams += [(ref.compress_fast(v), len(v)), (ref.compress_hc(v, 12), len(v))]
    out = []
    for s, d in streams:
        for t in targets_for(d, rng, n_random=1):
            for c in caps_for(t, rng):
                out.append((s, t, c))
    for s, d in streams[:6]:
        for _ in range(8):
            cut = rng.randrange(len(s) + 1)
            out.append((s[:cut], d, d))
            out.append((s[:cut], rng.randrange(d + 1), d))
    small = ref.compress_fast(book1[:300])
    out += [(small[:k], 400, 400) for k in range(len(small) + 1)]
    for off in range(1, 16):
        s, d = overlap_stream(rng, off)
        out += [(s, t, t + 3) for t in range(0, d + 2, 7)]
    for s, d in streams[:4]:
        out += [(damaged(s, rng, 2), rng.randrange(d + 5), d) for _ in range(20)]
    out += [(rng.randbytes(rng.randrange(0, 200)), rng.randrange(0, 300), 300) for _ in range(100)]
    out += [(b"", 0, 0), (b"", 5, 5), (b"\x00", 5, 5), (b"\x00", 0, 3), (b"\xff" * 10, 0, 10)]
    return out


@pytest.fixture(scope="module")
def want(cases, lz4p):
    return [lz4p(s, t, c) for s, t, c in cases]


def layout(cases):
    """one source buffer, one destination buffer with GUARD bytes between slots"""
    so, do, p, q = [], [], 0, 0
    for s, t, c in cases:
        so.append(p); do.append(q); p += len(s); q += c + GUARD
    return b"".join(s for s, _, _ in cases), so, do, q


def check(cases, want, got, dst, do, what, exact_tail=True):
    for i, ((s, t, c), (r, b)) in enumerate(zip(cases, want)):
        assert int(got[i]) == r, (what, i, len(s), t, c, int(got[i]), r)
        room = min(t, c)
        slot = bytes(dst[do[i]:do[i] + c + GUARD])
        assert same_bytes(slot[:max(r, 0)], b, s, r, room), (what, "bytes", i, len(s), t, c)
        tail = slot[max(r, 0) if exact_tail else room:]
        assert tail == b"\xee" * len(tail), (what, "written past the result" if exact_tail else "written past min(target, cap)", i, t, c)


def test_partial_host_batch(amd, cases, want):
    src, so, do, q = layout(cases)
    dst = bytearray(b"\xee" * q)
    got = amd.LZ4HIPBatch.decompressSafePartial(src, so, [len(s) for s, _, _ in cases], dst, do, [t for _, t, _ in cases],
                                                [c for _, _, c in cases])
    check(cases, want, got, dst, do, "host batch")   # (the host path hands back exactly the decoded bytes)


def test_partial_device_batch(amd, cases, want):
    import torch
    src, so, do, q = layout(cases)
    dev = torch.device("cuda", 0)
    d_src = torch.frombuffer(bytearray(src + b"\0"), dtype=torch.uint8).to(dev)
    d_dst = torch.full((q,), 0xEE, dtype=torch.uint8, device=dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    out = torch.full((len(cases),), -12345, dtype=torch.int32, device=dev)
    amd.DeviceBatch.decompress_safe_partial(d_src, i64(so), i32([len(s) for s, _, _ in cases]), d_dst, i64(do), i32([t for _, t, _ in cases]),
                                            i32([c for _, _, c in cases]), out)
    torch.cuda.synchronize()
    check(cases, want, out.cpu().tolist(), bytearray(d_dst.cpu().numpy().tobytes()), do, "device batch", exact_tail=False)


def test_partial_single_calls_coalesced_from_threads(amd, cases, want):
    d = amd.LZ4Factory.hipInstance().safeDecompressor()
    pick = list(range(0, len(cases), 3))

    def one(i):
        s, t, c = cases[i]
        buf = bytearray(b"\xee" * (c + GUARD + 3))
        try:
            r = d.decompressPartial(s, 0, len(s), buf, 3, t, c)
        except amd.LZ4Exception as e:
            return i, ("error", str(e)), buf
        return i, r, buf

    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, pick))
    for i, r, buf in res:
        s, t, c = cases[i]
        wr, wb = want[i]
        if wr < 0:
            assert r == ("error", "Error decoding offset %d of input buffer" % (-wr)), (i, r, wr)
            assert bytes(buf[3 + min(t, c):]) == b"\xee" * (c + GUARD - min(t, c))
        else:
            assert r == wr, (i, len(s), t, c, r, wr)
            assert same_bytes(bytes(buf[3:3 + r]), wb, s, wr, min(t, c)), (i, t, c)
            assert bytes(buf[3 + r:]) == b"\xee" * (len(buf) - 3 - r)
        assert buf[:3] == b"\xee\xee\xee"


def test_partial_both_kernels_ragged_targets(amd, ref, O, lz4p):
    """40959 blocks (the deep kernel) and 40960 (the staged kernel): small blocks whose neighbours in a wavefront get target 0, tiny
    targets, cuts inside a match and the whole block"""
    rng = rng_for(22)
    book1 = calgary("book1")
    base = [ref.compress_fast(book1[k * 700:k * 700 + 2000]) for k in range(8)] + [ref.compress_hc(O.gen_block(2000, 5), 12),
                                                                                    ref.compress_fast(bytes(2000))]
    for n in (40959, 40960):
        idx = [i % len(base) for i in range(n)]
        tclass = [(0, 1, 5, 13, 700, 2000, 1999, 3000)[rng.randrange(8)] if i % 5 else rng.randrange(2001) for i in range(n)]
        caps = [t if i % 3 == 0 else 2000 for i, t in enumerate(tclass)]
        cache = {}
        want = []
        for b, t, c in zip(idx, tclass, caps):
            if (b, t, c) not in cache:
                cache[(b, t, c)] = lz4p(base[b], t, c)
            want.append(cache[(b, t, c)])
        src = b"".join(base)
        boff = np.cumsum([0] + [len(s) for s in base])[:-1]
        so = np.array([boff[b] for b in idx], dtype=np.uint64)
        sl = np.array([len(base[b]) for b in idx], dtype=np.int32)
        do = np.arange(n, dtype=np.uint64) * np.uint64(2000 + GUARD)
        dst = bytearray(b"\xee" * (n * (2000 + GUARD)))
        got = amd.LZ4HIPBatch.decompressSafePartial(src, so, sl, dst, do, np.array(tclass, dtype=np.int32), np.array(caps, dtype=np.int32))
        for i in range(n):
            r, b = want[i]
            assert int(got[i]) == r, (n, i, tclass[i], caps[i], int(got[i]), r)
            o = int(do[i])
            assert bytes(dst[o:o + r]) == b, (n, i)
            assert dst[o + r:o + 2000 + GUARD] == b"\xee" * (2000 + GUARD - r), (n, i)


def test_partial_negative_sizes_and_edges(amd):
    """a negative src_len, target or capacity gives -1 (the engine's rule) in the host batch, the device batch and the single call"""
    l = amd.lib()
    s = (C.c_uint8 * 8)(0x10, 0x61, 0, 0, 0, 0, 0, 0)
    rows = [(2, -1, 10), (2, 10, -1), (-1, 10, 10), (-5, 0, 0), (2, -7, -7), (2, 1, 10), (2, 0, 10), (0, 5, 5), (0, 0, 5)]
    expect = [-1, -1, -1, -1, -1, 1, 0, -1, 0]
    n = len(rows)
    so, do = (C.c_uint64 * n)(*([0] * n)), (C.c_uint64 * n)(*[16 * i for i in range(n)])
    sl, tl, dc = (C.c_int32 * n)(*[r[0] for r in rows]), (C.c_int32 * n)(*[r[1] for r in rows]), (C.c_int32 * n)(*[r[2] for r in rows])
    dst, out = (C.c_uint8 * (16 * n))(*([0xEE] * 16 * n)), (C.c_int32 * n)()
    assert l.lz4hip_decompress_safe_partial_batch(s, so, sl, dst, do, tl, dc, out, n) == 0
    assert list(out) == expect
    assert bytes(dst[16 * 5:16 * 5 + 16]) == b"a" + b"\xee" * 15
    assert all(bytes(dst[16 * i:16 * i + 16]) == b"\xee" * 16 for i in range(n) if i != 5)
    for (a, b, c), e in zip(rows, expect):
        d1 = (C.c_uint8 * 16)(*([0xEE] * 16))
        assert l.lz4hip_decompress_safe_partial(s, a, d1, b, c) == e
    import torch
    dev = torch.device("cuda", 0)
    t = lambda arr, ty: torch.tensor(list(arr), dtype=ty, device=dev)
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    d_dst = torch.full((16 * n,), 0xEE, dtype=torch.uint8, device=dev)
    amd.DeviceBatch.decompress_safe_partial(t(s, torch.uint8), t(so, torch.int64), t(sl, torch.int32), d_dst, t(do, torch.int64),
                                            t(tl, torch.int32), t(dc, torch.int32), d_out)
    torch.cuda.synchronize()
    assert d_out.cpu().tolist() == expect


def test_partial_long_literal_run(amd, lz4p):
    """token 0xF0, 8.5 MB of 0xFF, 0x10, 104 letters: the run's 32-bit length sum passes 2^31; cut to the input (104 bytes) by the
    partial decoder, an error for the full decoder -- on both kernels' batch sizes' paths (host batch, device batch, single call)"""
    s, letters = long_literal_stream()
    assert lz4p(s, 1000, 1000) == (104, letters)
    assert lz4p(s, 50, 1000) == (50, letters[:50])
    rows = [(1000, 1000), (50, 1000), (1000, 60)]
    n = len(rows)
    dst = bytearray(b"\xee" * (n * 1008))
    got = amd.LZ4HIPBatch.decompressSafePartial(s, [0] * n, [len(s)] * n, dst, [1008 * i for i in range(n)], [r[0] for r in rows],
                                                [r[1] for r in rows])
    assert got == [104, 50, 60]
    assert bytes(dst[:104]) == letters and bytes(dst[1008:1058]) == letters[:50] and bytes(dst[2016:2076]) == letters[:60]
    assert amd.LZ4HIPBatch.decompressSafe(s, [0], [len(s)], bytearray(1000), [0], [1000])[0] < 0
    buf = bytearray(1000)
    assert amd.LZ4SafeDecompressor().decompressPartial(s, 0, len(s), buf, 0, 1000) == 104 and bytes(buf[:104]) == letters


def test_partial_issue_examples(amd, ref, lz4p):
    """book1's first 64 KiB: any target T returns T; a target above the size returns 65536; target 5000 with capacity 3000 returns
    3000; the first 100 compressed bytes decode to 97 bytes, half the stream to 31922"""
    v = calgary("book1")[:65536]
    s = ref.compress_fast(v)
    d = amd.LZ4SafeDecompressor()
    for t in (1, 100, 4096, 65535, 65536, 70000):
        buf = bytearray(b"\xee" * 70010)
        r = d.decompressPartial(s, 0, len(s), buf, 0, t)
        assert r == min(t, 65536) == lz4p(s, t, 70010)[0] and bytes(buf[:r]) == v[:r] and buf[r:] == b"\xee" * (70010 - r)
    assert d.decompressPartial(s, 0, len(s), bytearray(3000), 0, 5000) == 3000
    assert d.decompressPartial(s, 0, 100, bytearray(65536), 0, 65536) == 97 == lz4p(s[:100], 65536, 65536)[0]
    assert d.decompressPartial(s, 0, len(s) // 2, bytearray(65536), 0, 65536) == lz4p(s[:len(s) // 2], 65536, 65536)[0]
    # the full decoder rejects what the partial one returns
    with pytest.raises(amd.LZ4Exception):
        d.decompress(s, 0, len(s), bytearray(4096), 0, 4096)


def test_partial_cpp_mirror(tmp_path, cases, want):
    exe = build_mirror("partial_mirror_test", tmp_path)
    for i in range(0, len(cases), max(1, len(cases) // 25)):
        s, t, c = cases[i]
        wr, wb = want[i]
        sp, op = tmp_path / "s.bin", tmp_path / "o.bin"
        sp.write_bytes(s)
        p = subprocess.run([exe, str(sp), str(t), str(c), str(op)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (i, p.stderr)
        line = p.stdout.decode().strip()
        if wr < 0:
            assert line == "error Error decoding offset %d of input buffer" % (3 - wr), (i, line, wr)
        else:
            assert int(line) == wr and same_bytes(op.read_bytes(), wb, s, wr, min(t, c)), (i, line, wr)


def test_partial_jni_shim(tmp_path, cases, want):
    exe = build_fake_jni("fake_jni_partial", tmp_path)
    picked = [i for i in range(0, len(cases), max(1, len(cases) // 20)) if len(cases[i][0]) > 0]
    for i in picked:
        s, t, c = cases[i]
        wr, wb = want[i]
        sp = tmp_path / "s.bin"
        sp.write_bytes(s)
        out = subprocess.check_output([exe, str(sp), str(t), str(c), str(tmp_path)], timeout=120).decode()
        assert "checks ok" in out, out
        assert int((tmp_path / "partial.txt").read_text()) == wr, (i, wr)
        if wr > 0:
            assert same_bytes((tmp_path / "partial.bin").read_bytes(), wb, s, wr, min(t, c)), i


def test_partial_multidev_host_path():
    """lz4hip_init([0] * 2): the host batch takes the multi-device branch (block ranges per listed device)"""
    assert "partial multidev ok D=2" in run_child("partial_multidev_child.py", "2", timeout=600)
