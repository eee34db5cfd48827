"""The two variants of the block host path's metadata beyond one chunk (-m gpu): LZ4HIPBatch.compressDestSize, whose consumed sizes
travel behind the results, and LZ4HIPBatch.decompressedLengths, which has no destination buffer at all.  With 1 MiB chunks
(LZ4HIP_HOST_CHUNK_MB=1, read per call) 56 ragged blocks of 0 .. 64 KiB are staged in three chunks or more on rotating buffer sets;
every value and byte is the reference library's (LZ4_compress_destSize, LZ4_decompress_safe)."""
import random

import numpy as np
import pytest

from conftest import calgary
from size_common import ref_size
from support import offsets
from test_gpu_destsize import GUARD, bound, lz4dest  # noqa: F401 -- lz4dest is a fixture

pytestmark = pytest.mark.gpu
N_BLOCKS = 56


def ragged_blocks(O):
    """56 blocks of 0 .. 64 KiB, most of them large: text, numbers, an image, synthetic, incompressible"""
    rng = random.Random(61)
    book1, geo, pic = calgary("book1"), calgary("geo"), calgary("pic")
    sizes = [0, 1, 12, 13, 700, 65536, 65535] + [rng.randrange(48000, 65537) for _ in range(N_BLOCKS - 7)]
    rng.shuffle(sizes)
    out = []
    for k, n in enumerate(sizes):
        kind = k % 5
        if kind == 0:
            o = rng.randrange(len(book1) - n); v = book1[o:o + n]
        elif kind == 1:
            o = rng.randrange(len(geo) - n); v = geo[o:o + n]
        elif kind == 2:
            o = rng.randrange(len(pic) - n); v = pic[o:o + n]
        elif kind == 3:
            v = O.gen_block(n, k)
        else:
            v = rng.randbytes(n)
        out.append(v)
    return out, rng


def rounded(lengths):
    return sum((n + 15) & ~15 for n in lengths)


def test_dest_size_host_batch_in_small_chunks(amd, ref, lz4dest, O, monkeypatch):  # noqa: F811
    """out[] and consumed[] of every chunk land at their blocks; only the bytes written come back, the rest of every slot stays"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    blocks, rng = ragged_blocks(O)
    assert len(blocks) == N_BLOCKS and rounded(len(v) for v in blocks) > 2 << 20      # three chunks at least
    targets = []
    for k, v in enumerate(blocks):
        dl = len(ref.compress_fast(v))
        targets.append((dl, max(dl - 1, 1), max(dl // 2, 1), bound(len(v)), 17, rng.randrange(1, bound(len(v)) + 1))[k % 6])
    gap = 32
    so = offsets([len(v) for v in blocks])
    do = offsets([t + gap for t in targets])
    dst = bytearray([GUARD]) * (int(do[-1]) + targets[-1] + gap)
    out, cons = amd.LZ4HIPBatch.compressDestSize(b"".join(blocks) + b"\0", so, np.array([len(v) for v in blocks], dtype=np.int32), dst, do,
                                                 np.array(targets, dtype=np.int32))
    for k, (v, t) in enumerate(zip(blocks, targets)):
        r, used, by = lz4dest(v, t)
        o = int(do[k])
        assert (int(out[k]), int(cons[k])) == (r, used), (k, len(v), t, int(out[k]), int(cons[k]), r, used)
        assert bytes(dst[o:o + r]) == by, (k, len(v), t)
        assert dst[o + r:o + t + gap] == bytearray([GUARD]) * (t + gap - r), ("guard", k, t)


def test_decoded_size_host_batch_in_small_chunks(amd, ref, O, monkeypatch):
    """no destination exists on either side: the streams go up in three chunks or more, out[] comes back per chunk"""
    monkeypatch.setenv("LZ4HIP_HOST_CHUNK_MB", "1")
    blocks, rng = ragged_blocks(O)
    want = ref_size(ref)
    streams, caps = [], []
    for k, v in enumerate(blocks):
        s = ref.compress_fast(v if k % 5 < 2 else rng.randbytes(len(v)))        # (most streams large: the chunks are cut by stream bytes)
        if k % 7 == 3 and len(s) > 20:
            s = s[:rng.randrange(1, len(s))]                                    # truncated: a negative result
        streams.append(s)
        caps.append((len(v), len(v) + 64, max(len(v) - 1, 0), 65, 8 << 20)[k % 5])
    assert len(streams) == N_BLOCKS and rounded(len(s) for s in streams) > 2 << 20    # three chunks at least
    got = amd.LZ4HIPBatch.decompressedLengths(b"".join(streams) + b"\0", offsets([len(s) for s in streams]),
                                              np.array([len(s) for s in streams], dtype=np.int32), np.array(caps, dtype=np.int32))
    w = [want(s, c) for s, c in zip(streams, caps)]
    assert [int(g) for g in got] == w
    assert sum(1 for v in w if v < 0) >= 8 and sum(1 for v in w if v > 0) >= 20
