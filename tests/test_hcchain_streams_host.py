"""LZ4FrameOutputStream(linkedBlocks=True, level=N) (lz4-java_amd/streams.py) on the CPU: the writer's logic -- no block-independence
flag, every batch one HC chain behind the last 64 KB written, stored blocks that still count as history, checksums, host assembly --
with a test-side oracle engine whose compressHCChain is the reference library's LZ4_compress_HC_continue
(hcchain_common.oracle_hcchain_engine).  The frame must equal, byte for byte, the frame assembled here from ONE reference stream over
the whole data, whatever batchBlocks is, and read back through LZ4FrameInputStream(linkedBlocks=True); level=None writes what it
writes today."""
import importlib
import io
import random

import pytest

import streams_common as sc
from chain_common import RefChain, oracle_chain_engine
from cchain_common import RefCChain, batched_linked_frame, book1, oracle_cchain_engine
from hcchain_common import RefHCChain, hc_linked_frame, oracle_hcchain_engine


@pytest.fixture(scope="module")
def S(amd):
    return importlib.import_module("lz4-java_amd.streams")


@pytest.fixture(scope="module")
def rh(ref):
    return RefHCChain(ref)


@pytest.fixture(scope="module")
def rc(ref):
    return RefCChain(ref)


@pytest.fixture(scope="module")
def engine(port, O, ref, rc, rh):
    """compressHCChain, compressFastChain and decompressSafeChain, all served by the reference library"""
    base = type(oracle_chain_engine(sc.OracleEngine, RefChain(ref), port=port, O=O))
    base = type(oracle_cchain_engine(base, rc, port=port, O=O))
    return oracle_hcchain_engine(base, rh, port=port, O=O)


@pytest.fixture(scope="module")
def data():
    """text, a run that does not compress (stored blocks in the middle of the stream), text that repeats what lay in front of it"""
    b = book1()
    return b[:300000] + random.Random(9).randbytes(150000) + b[250000:420000]


def write(S, engine, data, block_id, batch, bits=(), pieces=None, level=9):
    sink = io.BytesIO()
    w = S.LZ4FrameOutputStream(sink, block_id, -1, *bits, engine=engine, batchBlocks=batch, linkedBlocks=True, level=level)
    for a in range(0, len(data), pieces or len(data)):
        w.write(data[a:a + (pieces or len(data))])
    w.close()
    return sink.getvalue()


def read_all(S, frame, engine, batch=64):
    return S.LZ4FrameInputStream(io.BytesIO(frame), engine=engine, batchBlocks=batch, linkedBlocks=True).read()


def test_the_frame_does_not_depend_on_batch_blocks(S, engine, rh, port, data):
    """batchBlocks 1, 3 and 64, whole writes and pieces: one frame, the reference's; the reader gives the data back"""
    B = S.FLG.Bits
    for block_id, level in ((4, 9), (5, 3), (4, 10)):
        d = data if level < 10 else data[:260000]
        want = hc_linked_frame(rh, port.xxh32, d, block_id, level, block_checksum=True, content_checksum=True)
        for batch in (1, 3, 64):
            c0 = engine.hcchain_calls
            got = write(S, engine, d, block_id, batch, (B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM), pieces=batch << (2 * block_id + 8), level=level)
            assert got == want, (block_id, level, batch)
            assert got[4] & 0x20 == 0 and engine.hcchain_calls - c0 >= (len(d) >> (2 * block_id + 8)) // batch
        assert write(S, engine, d, block_id, 64, (B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, B.BLOCK_INDEPENDENCE), pieces=70001, level=level) == want
        for rb in (1, 64):
            assert read_all(S, want, engine, rb) == d
    # stored blocks in the middle, and the HC frame is smaller than the fast chain's
    want = hc_linked_frame(rh, port.xxh32, data, 4, 9)
    assert write(S, engine, data, 4, 64) == want
    assert len(want) < len(write(S, engine, data, 4, 64, level=None))


def test_level_none_writes_what_it_writes_today(S, engine, rc, port, data):
    """the default is the fast chain: batches are visible in its bytes, as before"""
    for batch in (3, 64):
        want = batched_linked_frame(rc, port.xxh32, data, 4, batch)
        assert write(S, engine, data, 4, batch, pieces=batch << 16, level=None) == want
        sink = io.BytesIO()
        w = S.LZ4FrameOutputStream(sink, 4, -1, engine=engine, batchBlocks=batch, linkedBlocks=True)
        for a in range(0, len(data), batch << 16):
            w.write(data[a:a + (batch << 16)])
        w.close()
        assert sink.getvalue() == want


def test_flush_cuts_a_short_block_and_the_chain_goes_on(S, engine, data):
    sink = io.BytesIO()
    w = S.LZ4FrameOutputStream(sink, 4, -1, engine=engine, batchBlocks=64, linkedBlocks=True, level=9)
    w.write(data[:100000]); w.flush()
    w.write(data[100000:100010]); w.flush()
    w.write(data[100010:]); w.close()
    assert read_all(S, sink.getvalue(), engine) == data


def test_level_needs_linked_blocks_and_an_engine_that_has_them(S, engine, port, O):
    plain = sc.OracleEngine(port, O)
    with pytest.raises(ValueError):
        S.LZ4FrameOutputStream(io.BytesIO(), 4, -1, engine=engine, level=9)                      # independent blocks have no chain level
    with pytest.raises(ValueError):
        S.LZ4FrameOutputStream(io.BytesIO(), 4, -1, engine=plain, linkedBlocks=True, level=9)
    assert hasattr(S.HIPEngine, "compressHCChain")
    doc = S.LZ4FrameOutputStream.__doc__
    assert "DO NOT DEPEND ON batchBlocks" in doc and "one wavefront" in doc
