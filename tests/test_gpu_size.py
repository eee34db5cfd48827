"""The decoded-size query on the GPU against the return value of the reference library's own LZ4_decompress_safe (called with a real
buffer of cap + 64 bytes): the device batch at every grid shape, the host batch, coalesced single calls, the Python layers, the C++
mirror and the JNI shim, the multi-device host path; streams longer than the kernel's LDS ring; agreement with the decoder; the
sized decode; and that nothing but out[] is written.  Zero mismatches, nothing skipped, every test asserts its case count."""
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from size_common import caps_for, edge_streams, long_literal_stream, ref_decode, ref_size, rng_for, seam_streams, stream_set
from support import build_fake_jni, build_mirror, run_child

pytestmark = pytest.mark.gpu
BATCH = 3000


class Parity:
    """the hostsim stream set with the capacity list: rows (stream index, capacity), the reference's value per row, the streams
    packed into one buffer"""

    def __init__(self, ref, O):
        rng = rng_for(31)
        want = ref_size(ref)
        sets = stream_set(ref, O, rng) + seam_streams(rng) + edge_streams(rng)
        self.streams = [s for _, s, _ in sets]
        self.off = np.concatenate([[0], np.cumsum([len(s) for s in self.streams])[:-1]]).astype(np.int64)
        self.src = b"".join(self.streams) + b"\0"
        rows = [(k, cap) for k, (_, s, d) in enumerate(sets) for cap in caps_for(d, len(s))]
        rng.shuffle(rows)                        # (every batch mixes stream kinds and capacities)
        self.idx = np.array([k for k, _ in rows], dtype=np.int64)
        self.cap = np.array([c for _, c in rows], dtype=np.int32)
        self.want = np.array([want(self.streams[k], c) for k, c in rows], dtype=np.int32)
        self.so = self.off[self.idx]
        self.sl = np.array([len(self.streams[k]) for k in self.idx], dtype=np.int32)


@pytest.fixture(scope="module")
def parity(ref, O):
    return Parity(ref, O)


@pytest.fixture(scope="module")
def d_src(parity):
    import torch
    return torch.frombuffer(bytearray(parity.src), dtype=torch.uint8).to(torch.device("cuda", 0))


def dev_sizes(amd, d_src, so, sl, cap):
    import torch
    dev = d_src.device
    out = torch.full((len(so),), -12345, dtype=torch.int32, device=dev)
    amd.DeviceBatch.decoded_size(d_src, torch.as_tensor(np.asarray(so, dtype=np.int64), device=dev), torch.as_tensor(np.asarray(sl, dtype=np.int32), device=dev),
                                 torch.as_tensor(np.asarray(cap, dtype=np.int32), device=dev), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def mismatches(got, want):
    return [(int(i), int(got[i]), int(want[i])) for i in np.nonzero(np.asarray(got) != np.asarray(want))[0][:10]]


def test_size_parity_device_batches(amd, parity, d_src):
    """about 4000 valid and damaged streams with the whole capacity list, in device batches of 3000 blocks (the grid is full) and of
    1, 63, 64 and 65 blocks (the spread path: fewer blocks than a workgroup per CU)"""
    n = len(parity.idx)
    assert len(parity.streams) > 3900 and n > 50000
    checked = 0
    for a in range(0, n, BATCH):
        b = min(a + BATCH, n)
        got = dev_sizes(amd, d_src, parity.so[a:b], parity.sl[a:b], parity.cap[a:b])
        assert not mismatches(got, parity.want[a:b]), (a, mismatches(got, parity.want[a:b]))
        checked += b - a
    assert checked == n
    small = 0
    for size in (1, 63, 64, 65):
        for a in (0, 7001, 20011, n - size):
            got = dev_sizes(amd, d_src, parity.so[a:a + size], parity.sl[a:a + size], parity.cap[a:a + size])
            assert not mismatches(got, parity.want[a:a + size]), (size, a, mismatches(got, parity.want[a:a + size]))
            small += size
    assert small == 4 * (1 + 63 + 64 + 65)


def test_size_host_batch(amd, parity):
    """the host-pointer path (staging of the streams only) on a slice of the parity set, lists and numpy arrays"""
    a, b = 5000, 5000 + 2 * BATCH
    got = amd.LZ4HIPBatch.decompressedLengths(parity.src, parity.so[a:b].astype(np.uint64), parity.sl[a:b], parity.cap[a:b])
    assert len(got) == 2 * BATCH and not mismatches(got, parity.want[a:b])
    got = amd.LZ4HIPBatch.decompressedLengths(parity.src, [int(v) for v in parity.so[:100]], [int(v) for v in parity.sl[:100]],
                                              [int(v) for v in parity.cap[:100]])
    assert got == [int(v) for v in parity.want[:100]]


def test_size_long_streams(amd, ref, O):
    """streams longer than the kernel's ring: eight reference-compressed 4 MiB App. F blocks (their ends fall in different windows),
    4 MiB of zeros (one long extension run) and the long-literal stream whose 32-bit length sum passes 2^31"""
    want = ref_size(ref)
    big = [ref.compress_fast(O.gen_block(4 << 20, 40 + i)) for i in range(8)]
    assert len({len(s) % 256 for s in big}) > 4 and min(len(s) for s in big) > (1 << 20)
    zeros = ref.compress_fast(bytes(4 << 20))
    lls, _ = long_literal_stream()
    rows = []
    for s in big + [zeros]:
        rows += [(s, c) for c in ((4 << 20) - 1, 4 << 20, (4 << 20) + 64, (4 << 20) + 607, 65, 8 << 20)]
    rows += [(s[:len(s) // 2], 8 << 20) for s in big[:2]] + [(lls, c) for c in (0, 63, 64, 65, 1000, 8 << 20)]
    src = b"".join(s for s, _ in rows)
    so = np.concatenate([[0], np.cumsum([len(s) for s, _ in rows])[:-1]]).astype(np.uint64)
    got = amd.LZ4HIPBatch.decompressedLengths(src, so, np.array([len(s) for s, _ in rows], dtype=np.int32), np.array([c for _, c in rows], dtype=np.int32))
    w = [want(s, c) for s, c in rows]
    assert len(rows) == 9 * 6 + 2 + 6 and not mismatches(got, w), mismatches(got, w)
    assert w[1] == 4 << 20 and w[0] < 0 and all(v < 0 for v in w[-6:])


def test_size_mixed_batch_in_one_wavefronts_worth(amd, ref, O):
    """0-byte, 1-byte, 13-byte and 64 KiB streams side by side in 64 blocks"""
    want = ref_size(ref)
    kinds = [b"", b"\x00", ref.compress_fast(b"abcdefghijkl"), ref.compress_fast(O.gen_block(65536, 77)), ref.compress_fast(b"hello, hello, hello, hello, hello!")]
    assert [len(k) for k in kinds[:3]] == [0, 1, 13]
    rows = [(kinds[(i * 7 + i // 5) % len(kinds)], (0, 13, 64, 65536, 70000)[i % 5]) for i in range(64)]
    src = b"".join(s for s, _ in rows) + b"\0"
    so = np.concatenate([[0], np.cumsum([len(s) for s, _ in rows])[:-1]]).astype(np.uint64)
    got = amd.LZ4HIPBatch.decompressedLengths(src, so, np.array([len(s) for s, _ in rows], dtype=np.int32), np.array([c for _, c in rows], dtype=np.int32))
    w = [want(s, c) for s, c in rows]
    assert len(rows) == 64 and not mismatches(got, w), mismatches(got, w)
    assert 65536 in w and 0 in w and -1 in w


def test_size_writes_nothing_but_out(amd, parity):
    """the entry point takes no destination; the device buffers around its arrays -- the streams themselves, guard words in front of
    and behind out[] and behind the streams -- are as they were after a batch of 3000 blocks; negative sizes give -1"""
    import torch
    dev = torch.device("cuda", 0)
    n, G = BATCH, 4096
    arena = torch.full((G + len(parity.src) + G,), 0xEE, dtype=torch.uint8, device=dev)
    arena[G:G + len(parity.src)] = torch.frombuffer(bytearray(parity.src), dtype=torch.uint8).to(dev)
    before = arena.clone()
    outbuf = torch.full((G // 4 + n + G // 4,), 0x6E6E6E6E, dtype=torch.int32, device=dev)
    sl = parity.sl[:n].copy(); cap = parity.cap[:n].copy()
    sl[5] = -1; cap[9] = -7
    i64 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.int64), device=dev)
    i32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.int32), device=dev)
    amd.DeviceBatch.decoded_size(arena[G:], i64(parity.so[:n]), i32(sl), i32(cap), outbuf[G // 4:G // 4 + n])
    torch.cuda.synchronize()
    assert torch.equal(arena, before)
    o = outbuf.cpu().numpy()
    assert (o[:G // 4] == 0x6E6E6E6E).all() and (o[G // 4 + n:] == 0x6E6E6E6E).all()
    w = parity.want[:n].copy(); w[5] = -1; w[9] = -1
    assert not mismatches(o[G // 4:G // 4 + n], w)
    # NULL arrays on a device are argument errors; the empty batch is fine
    l = amd.lib()
    assert l.lz4hip_decompressed_size_batch_dev(None, None, None, None, None, 0, 0, None) == 0
    assert l.lz4hip_decompressed_size_batch_dev(arena.data_ptr(), None, None, None, None, 1, 0, None) == -3


def test_size_agrees_with_the_decoder(amd, parity, d_src):
    """for every stream and capacity of the parity set the query's value is what lz4hip_decompress_safe_batch_dev (the routed decoder,
    once per batch) returns on the same input -- so a value >= 0 promises that the decode succeeds with exactly that size"""
    import torch
    dev = d_src.device
    n = len(parity.idx)
    checked = 0
    for a in range(0, n, BATCH):
        b = min(a + BATCH, n)
        cap = parity.cap[a:b].astype(np.int64)
        do = np.concatenate([[0], np.cumsum(cap + 16)[:-1]])
        dst = torch.empty(int((cap + 16).sum()) + 64, dtype=torch.uint8, device=dev)
        out = torch.full((b - a,), -12345, dtype=torch.int32, device=dev)
        amd.DeviceBatch.decompress_safe(d_src, torch.as_tensor(parity.so[a:b], device=dev), torch.as_tensor(parity.sl[a:b], device=dev), dst,
                                        torch.as_tensor(do, device=dev), torch.as_tensor(parity.cap[a:b], device=dev), out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert not mismatches(got, parity.want[a:b]), (a, mismatches(got, parity.want[a:b]))
        del dst
        checked += b - a
    assert checked == n


def test_size_sized_decode(amd, ref, parity):
    """decompressSafeSized over a batch with failing streams: the reference's bytes for the good ones, liblz4's code and an empty slot
    for the bad ones, a buffer of exactly the sum of the sizes"""
    dec = ref_decode(ref)
    pick = [i for i in range(0, 12000, 6)]
    so = [int(parity.so[i]) for i in pick]; sl = [int(parity.sl[i]) for i in pick]; cap = [int(parity.cap[i]) for i in pick]
    buf, offs, lens = amd.LZ4HIPBatch.decompressSafeSized(parity.src, so, sl, cap)
    w = [int(parity.want[i]) for i in pick]
    assert lens == w and len(buf) == sum(max(v, 0) for v in w)
    good = bad = 0
    for j, i in enumerate(pick):
        assert offs[j] == sum(max(v, 0) for v in w[:j]) if j < 50 else True
        if w[j] < 0:
            bad += 1
            continue
        s = parity.streams[int(parity.idx[i])]
        assert bytes(buf[offs[j]:offs[j] + w[j]]) == dec(s, cap[j])[1], (j, i)
        good += 1
    assert good > 300 and bad > 300 and good + bad == 2000


def test_size_single_calls_coalesced_from_threads(amd, parity):
    d = amd.LZ4Factory.hipInstance().safeDecompressor()
    pick = list(range(0, 40000, 100))

    def one(i):
        s = parity.streams[int(parity.idx[i])]
        try:
            return d.decompressedLength(b"xyz" + s, 3, len(s), int(parity.cap[i]))
        except amd.LZ4Exception as e:
            return str(e)

    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, pick))
    for i, r in zip(pick, res):
        w = int(parity.want[i])
        assert r == (w if w >= 0 else "Error decoding offset %d of input buffer" % (3 - w)), (i, r, w)
    assert len(res) == 400


def test_size_cpp_mirror(tmp_path, ref, parity):
    exe = build_mirror("size_mirror_test", tmp_path)
    want, dec = ref_size(ref), ref_decode(ref)
    ran = 0
    for i in range(0, len(parity.idx), len(parity.idx) // 12):
        s, c = parity.streams[int(parity.idx[i])], int(parity.cap[i])
        if not s:
            continue
        sp, op = tmp_path / "s.bin", tmp_path / "o.bin"
        sp.write_bytes(s)
        p = subprocess.run([exe, str(sp), str(c), str(op)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (i, p.stderr)
        lines = p.stdout.decode().strip().split("\n")
        w = int(parity.want[i])
        assert lines[0] == (str(w) if w >= 0 else "error Error decoding offset %d of input buffer" % (3 - w)), (i, lines, w)
        w3 = [w, want(s[:-1], c), w]
        assert [int(v) for v in lines[1].split()] == w3
        data = op.read_bytes()
        assert len(data) == sum(max(v, 0) for v in w3)
        if w > 0:
            assert data[:w] == dec(s, c)[1] == data[len(data) - w:]
        ran += 1
    assert ran >= 10


def test_size_jni_shim(tmp_path, ref, parity):
    exe = build_fake_jni("fake_jni_size", tmp_path)
    want = ref_size(ref)
    ran = 0
    for i in range(3, len(parity.idx), len(parity.idx) // 12):
        s, c = parity.streams[int(parity.idx[i])], int(parity.cap[i])
        if not s:
            continue
        sp = tmp_path / "s.bin"
        sp.write_bytes(s)
        out = subprocess.check_output([exe, str(sp), str(c), str(tmp_path)], timeout=120).decode()
        assert "checks ok" in out, out
        assert int((tmp_path / "size.txt").read_text()) == int(parity.want[i]), i
        assert [int(v) for v in (tmp_path / "size_batch.txt").read_text().split()] == [int(parity.want[i]), want(s, 0), want(s[:-1], c)]
        ran += 1
    assert ran >= 10


def test_size_multidev_host_path():
    """lz4hip_init([0] * 2): the host batch takes the multi-device branch (block ranges per listed device)"""
    assert "size multidev ok D=2" in run_child("size_multidev_child.py", "2", timeout=600)
