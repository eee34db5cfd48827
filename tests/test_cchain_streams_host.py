"""The opt-in linked-block path of LZ4FrameOutputStream (lz4-java_amd/streams.py, linkedBlocks=True) on the CPU: the writer's logic --
no block-independence flag, one chain per batch of blocks behind the last 64 KB written, stored blocks that still count as history,
checksums, host assembly -- with a test-side oracle engine whose compressFastChain is the reference library's stream compressor
(cchain_common.oracle_cchain_engine).  The frames must equal, byte for byte, frames assembled here from the reference, and read back
through LZ4FrameInputStream(linkedBlocks=True)."""
import importlib
import io
import random

import pytest

import streams_common as sc
from chain_common import RefChain, linked_frame, oracle_chain_engine
from cchain_common import RefCChain, batched_linked_frame, book1, oracle_cchain_engine


@pytest.fixture(scope="module")
def S(amd):
    return importlib.import_module("lz4-java_amd.streams")


@pytest.fixture(scope="module")
def rc(ref):
    return RefCChain(ref)


@pytest.fixture(scope="module")
def rd(ref):
    return RefChain(ref)


@pytest.fixture(scope="module")
def engine(port, O, rc, rd):
    """compressFastChain and decompressSafeChain, both served by the reference library"""
    base = type(oracle_chain_engine(sc.OracleEngine, rd, port=port, O=O))
    return oracle_cchain_engine(base, rc, port=port, O=O)


@pytest.fixture(scope="module")
def data():
    """text, a run that does not compress (stored blocks in the middle of a chain), text that repeats what lay in front of it"""
    b = book1()
    return b[:300000] + random.Random(9).randbytes(150000) + b[250000:420000]


def write(S, engine, data, block_id, batch, bits=(), pieces=None):
    sink = io.BytesIO()
    w = S.LZ4FrameOutputStream(sink, block_id, -1, *bits, engine=engine, batchBlocks=batch, linkedBlocks=True)
    if pieces is None:
        w.write(data)
    else:
        for a in range(0, len(data), pieces):
            w.write(data[a:a + pieces])
    w.close()
    return sink.getvalue()


def read_all(S, frame, engine, batch=64):
    return S.LZ4FrameInputStream(io.BytesIO(frame), engine=engine, batchBlocks=batch, linkedBlocks=True).read()


def test_one_batch_frame_is_the_references_linked_frame(S, engine, rd, port, data):
    """block ids 4 and 5, with and without block and content checksums: the frame of chain_common.linked_frame, byte for byte"""
    B = S.FLG.Bits
    for block_id in (4, 5):
        for bits, kw in (((), dict()), ((B.BLOCK_CHECKSUM,), dict(block_checksum=True)), ((B.CONTENT_CHECKSUM,), dict(content_checksum=True)),
                         ((B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, B.BLOCK_INDEPENDENCE), dict(block_checksum=True, content_checksum=True))):
            want, spans = linked_frame(rd, port.xxh32, data, block_id, **kw)
            assert block_id != 4 or (any(raw for _, _, raw in spans) and not all(raw for _, _, raw in spans))
            c0 = engine.cchain_calls
            got = write(S, engine, data, block_id, 64, bits)
            assert got == want, (block_id, kw)
            assert got[4] & 0x20 == 0 and engine.cchain_calls - c0 == 1
            assert read_all(S, got, engine) == data
            assert write(S, engine, data, block_id, 64, bits, pieces=70001) == want


def test_frame_written_in_several_batches(S, engine, rc, port, data):
    """batches of 1, 3 and 4 blocks: every batch is a chain whose prefix is the last 64 KB written before it"""
    B = S.FLG.Bits
    for block_id, batch in ((4, 1), (4, 3), (4, 4), (5, 2)):
        want = batched_linked_frame(rc, port.xxh32, data, block_id, batch, block_checksum=True, content_checksum=True)
        # (a batch is what one write hands over once `batch` full blocks are buffered: pieces of exactly that size)
        got = write(S, engine, data, block_id, batch, (B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM), pieces=batch << (2 * block_id + 8))
        assert got == want, (block_id, batch)
        for rb in (1, 3, 64):
            assert read_all(S, got, engine, rb) == data
    # a batch boundary is not invisible: the bytes differ from the one-chain frame's, and both decode
    assert batched_linked_frame(rc, port.xxh32, data, 4, 3) != batched_linked_frame(rc, port.xxh32, data, 4, 64)


def test_flush_cuts_a_short_block_and_the_chain_goes_on(S, engine, rc, port, data):
    sink = io.BytesIO()
    w = S.LZ4FrameOutputStream(sink, 4, -1, engine=engine, batchBlocks=64, linkedBlocks=True)
    w.write(data[:100000]); w.flush()
    w.write(data[100000:100010]); w.flush()
    w.write(data[100010:]); w.close()
    assert read_all(S, sink.getvalue(), engine) == data


def test_default_is_unchanged_and_engines_without_chains_refuse(S, engine, port, O, data):
    """linkedBlocks defaults to False: the bytes are today's; an engine that cannot compress chains is refused"""
    plain = sc.OracleEngine(port, O)
    a, b = io.BytesIO(), io.BytesIO()
    for sink, kw in ((a, dict()), (b, dict(linkedBlocks=False))):
        w = S.LZ4FrameOutputStream(sink, 4, -1, engine=plain, **kw)
        w.write(data[:200000]); w.close()
    assert a.getvalue() == b.getvalue() and a.getvalue()[4] & 0x20
    with pytest.raises(ValueError):
        S.LZ4FrameOutputStream(io.BytesIO(), 4, -1, engine=plain, linkedBlocks=True)
    assert hasattr(S.HIPEngine, "compressFastChain")
    assert "one wavefront" in S.LZ4FrameOutputStream.__doc__
