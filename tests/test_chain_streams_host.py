"""The opt-in linked-block path of LZ4FrameInputStream (lz4-java_amd/streams.py, linkedBlocks=True) on the CPU: the reader's logic --
the host walk of size words, one chain per batch of blocks, the carried 64 KB of history, stored blocks inside a chain, checksums, the
order in which defects surface, the messages -- with a test-side oracle engine whose decompressSafeChain is the reference library's
stream decoder (chain_common.oracle_chain_engine).  Frames: what the `lz4` command line writes without block independence (where it
is installed) and frames assembled here from chains the reference compressed."""
import importlib
import io
import struct

import pytest

import streams_common as sc
from chain_common import Chain, RefChain, book1, linked_frame, oracle_chain_engine, rng_for

BATCHES = (1, 3, 64)


@pytest.fixture(scope="module")
def S(amd):
    return importlib.import_module("lz4-java_amd.streams")


@pytest.fixture(scope="module")
def rc(ref):
    return RefChain(ref)


@pytest.fixture(scope="module")
def engine(port, O, rc):
    return oracle_chain_engine(sc.OracleEngine, rc, port=port, O=O)


@pytest.fixture(scope="module")
def data():
    """text, a run that does not compress (stored blocks in the middle of a chain), text that repeats what lay in front of it"""
    b = book1()
    return b[:300000] + rng_for(9).randbytes(150000) + b[250000:420000]


def read_all(S, frame, engine, batch, **kw):
    return S.LZ4FrameInputStream(io.BytesIO(frame), engine=engine, batchBlocks=batch, linkedBlocks=True, **kw).read()


def test_linked_frames_assembled_from_reference_chains(S, engine, rc, port, data):
    """64 KB blocks with and without block checksums, content checksum and size; every batch size (1: every block is a chain of its
    own that lives on the carried history alone)"""
    for kw in (dict(), dict(block_checksum=True), dict(content_checksum=True, content_size=True), dict(block_checksum=True, content_checksum=True)):
        frame, spans = linked_frame(rc, port.xxh32, data, 4, **kw)
        assert len(spans) == 10 and any(raw for _, _, raw in spans) and not all(raw for _, _, raw in spans)
        assert frame[4] & 0x20 == 0                                   # no BLOCK_INDEPENDENCE
        for batch in BATCHES:
            c0 = engine.chain_calls
            assert read_all(S, frame, engine, batch) == data, (kw, batch)
            assert engine.chain_calls - c0 == -(-len(spans) // batch)
    # the blocks really are linked: block 1 alone does not decode
    s = rc.compress_chain(data[:131072], 65536)[1][0]
    assert rc.plain(s, 65536) != 65536
    big = (book1() * 12)[:9000000]                                    # 4 MB blocks: three of them
    frame, spans = linked_frame(rc, port.xxh32, big, 7, content_size=True)
    assert len(spans) == 3
    for batch in BATCHES:
        assert read_all(S, frame, engine, batch) == big


@pytest.mark.skipif(sc.LZ4_CLI is None, reason="lz4 CLI not installed")
def test_linked_frames_of_the_command_line(S, engine, data):
    big = (book1() * 12)[:9000000]
    for args, d in ((["-1", "-B4", "-BD"], data), (["-B4", "-BD", "-BX"], data), (["-B7", "-BD", "--content-size"], big)):
        frame = sc.cli(args, d)
        assert frame[4] & 0x20 == 0, args
        for batch in BATCHES:
            assert read_all(S, frame, engine, batch) == d, (args, batch)
            assert read_all(S, frame, engine, batch, hostWalk=True) == d
        sc._expect(S, frame, "BLOCK_INDEPENDENCE", engine)            # the default still refuses the frame


def test_linked_frame_defects_surface_in_order(S, engine, rc, port, data):
    """a corrupted block k delivers the blocks before it, then raises the existing messages"""
    frame, spans = linked_frame(rc, port.xxh32, data, 4)
    k = 3
    assert not spans[k][2]
    off, n, _ = spans[k]
    streams = [(frame[o:o + m], raw, 65536) for o, m, raw in spans]
    rng = rng_for(12)
    while True:                                                       # a damage the reference rejects (most flips of a literal are accepted)
        bad = bytearray(frame)
        for _ in range(3):
            bad[off + rng.randrange(n)] = rng.randrange(256)
        chain = list(streams)
        chain[k] = (bytes(bad[off:off + n]), False, 65536)
        r = rc.decode(Chain("damaged", chain))[0][k]
        if r < 0:
            break
    for batch in BATCHES:
        sc._expect(S, bytes(bad), "Error decoding offset %d of input buffer" % -r, engine, delivered=data[:k * 65536], batchBlocks=batch, linkedBlocks=True)
    # with block checksums the same damage is a checksum mismatch, found before anything of that batch is decoded past it
    frame, spans = linked_frame(rc, port.xxh32, data, 4, block_checksum=True)
    bad = bytearray(frame)
    bad[spans[k][0] + 5] ^= 0x41
    for batch in BATCHES:
        sc._expect(S, bytes(bad), sc_msg(S, "BLOCK_HASH_MISMATCH"), engine, delivered=data[:k * 65536], batchBlocks=batch, linkedBlocks=True)
    # a wrong content checksum, a wrong content size, a frame cut inside block 2
    frame, spans = linked_frame(rc, port.xxh32, data, 4, content_checksum=True)
    sc._expect(S, frame[:-1] + bytes([frame[-1] ^ 1]), "Content checksum mismatch", engine, delivered=data, linkedBlocks=True)
    frame, spans = linked_frame(rc, port.xxh32, data, 4, content_size=True)
    wrong = bytearray(frame)
    wrong[6:14] = struct.pack("<Q", len(data) + 1)
    wrong[14] = (port.xxh32(bytes(wrong[4:14]), 0) >> 8) & 0xFF
    sc._expect(S, bytes(wrong), "Size check mismatch", engine, delivered=data, linkedBlocks=True)
    frame, spans = linked_frame(rc, port.xxh32, data, 4)
    for batch in BATCHES:
        sc._expect(S, frame[:spans[2][0] + 100], sc_msg(S, "PREMATURE_EOS"), engine, delivered=data[:2 * 65536], batchBlocks=batch, linkedBlocks=True)


def sc_msg(S, name):
    return getattr(S, name)


def test_default_and_engines_without_chains_refuse(S, engine, rc, port, O, data):
    frame, _ = linked_frame(rc, port.xxh32, data[:100000], 4)
    sc._expect(S, frame, "Dependent block stream is unsupported (BLOCK_INDEPENDENCE must be set)", engine)
    sc._expect(S, frame, "Dependent block stream is unsupported (BLOCK_INDEPENDENCE must be set)", engine, linkedBlocks=False)
    plain = sc.OracleEngine(port, O)                                  # an engine that cannot decode chains keeps the refusal
    assert not hasattr(plain, "decompressSafeChain")
    sc._expect(S, frame, "Dependent block stream is unsupported (BLOCK_INDEPENDENCE must be set)", plain, linkedBlocks=True)
    with pytest.raises(RuntimeError):
        S.FLG.fromByte(0x40)
    assert not S.FLG.fromByte(0x40, allowDependent=True).isEnabled(S.FLG.Bits.BLOCK_INDEPENDENCE)
    with pytest.raises(RuntimeError):
        S.FLG.fromByte(0x41, allowDependent=True)                     # every other check stays


def test_independent_frames_take_todays_paths(S, engine, data):
    """BLOCK_INDEPENDENCE set: the flag changes nothing, no chain call is made"""
    sink = io.BytesIO()
    w = S.LZ4FrameOutputStream(sink, S.BLOCKSIZE.SIZE_64KB, -1, S.FLG.Bits.BLOCK_INDEPENDENCE, S.FLG.Bits.CONTENT_CHECKSUM, engine=engine)
    w.write(data)
    w.close()
    c0 = engine.chain_calls
    for batch in BATCHES:
        assert read_all(S, sink.getvalue(), engine, batch) == data
    assert engine.chain_calls == c0
