"""streams.writeFrames / writeBlockStreams on the CPU: over an oracle-backed engine that implements containerBlocksMany with the
reference, and over one that lacks it (the per-payload fall-back).  Both equal the per-payload writers byte for byte for every flag
combination; the `lz4` command line reads the frames; readFrames / readBlockStreams take the results back."""
import importlib
import io
import itertools

import pytest

import container_write_many_common as wm
import streams_common as sc


@pytest.fixture(scope="module")
def S(amd):
    return importlib.import_module("lz4-java_amd.streams")


@pytest.fixture(scope="module")
def payloads(O, corpus):
    return [it[1] for it in wm.cases(O, corpus)]


def frame_alone(S, engine, p, blockSize, bits):
    sink = io.BytesIO()
    w = S.LZ4FrameOutputStream(sink, blockSize, len(p) if S.FLG.Bits.CONTENT_SIZE in bits else -1, *bits, engine=engine)
    w.write(p)
    w.close()
    return sink.getvalue()


def stream_alone(S, engine, p, blockSize):
    sink = io.BytesIO()
    w = S.LZ4BlockOutputStream(sink, blockSize, engine=engine)
    w.write(p)
    w.close()
    return sink.getvalue()


def flag_sets(S):
    B = S.FLG.Bits
    for r in range(4):
        for extra in itertools.combinations((B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, B.CONTENT_SIZE), r):
            yield (B.BLOCK_INDEPENDENCE,) + extra


@pytest.mark.parametrize("level", [0, 9])
def test_write_frames_equals_the_per_payload_writer(S, ref, O, payloads, level):
    plain, many = wm.oracle_engine(ref, O, level), wm.oracle_many_engine(S, ref, O, level)
    assert not hasattr(plain, "containerBlocksMany")
    for blockSize in (S.BLOCKSIZE.SIZE_64KB, S.BLOCKSIZE.SIZE_256KB):
        for bits in flag_sets(S):
            want = [frame_alone(S, plain, p, blockSize, bits) for p in payloads]
            calls = type(many).calls
            got = S.writeFrames(payloads, engine=many, blockSize=blockSize, bits=bits)
            assert type(many).calls == calls + 1                       # one many-call per call
            assert got == want, (blockSize, bits, [i for i, (g, w) in enumerate(zip(got, want)) if g != w])
            assert S.writeFrames(payloads, engine=plain, blockSize=blockSize, bits=bits) == want
    assert S.writeFrames([], engine=many) == [] and S.writeFrames([], engine=plain) == []
    assert S.writeFrames(payloads[:3], engine=many) == [frame_alone(S, plain, p, S.BLOCKSIZE.SIZE_4MB, (S.FLG.Bits.BLOCK_INDEPENDENCE,)) for p in payloads[:3]]


@pytest.mark.parametrize("blockSize", [64, 1000, 1024, 1025, 65536, 128 << 10])
def test_write_block_streams_equals_the_per_payload_writer(S, ref, O, payloads, blockSize):
    plain, many = wm.oracle_engine(ref, O), wm.oracle_many_engine(S, ref, O)
    some = [p for p in payloads if len(p) <= 40 * blockSize]
    want = [stream_alone(S, plain, p, blockSize) for p in some]
    calls = type(many).calls
    assert S.writeBlockStreams(some, engine=many, blockSize=blockSize) == want
    assert type(many).calls == calls + 1
    assert S.writeBlockStreams(some, engine=plain, blockSize=blockSize) == want
    assert S.writeBlockStreams([], engine=many) == []


def test_written_containers_are_read_back(S, ref, O, payloads):
    many, reader = wm.oracle_many_engine(S, ref, O), sc.OracleDeviceEngine(ref, O)
    B = S.FLG.Bits
    frames = S.writeFrames(payloads, engine=many, blockSize=S.BLOCKSIZE.SIZE_64KB, bits=(B.BLOCK_INDEPENDENCE, B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, B.CONTENT_SIZE))
    assert S.readFrames(frames, engine=reader) == [(p, None) for p in payloads]
    streams = S.writeBlockStreams(payloads, engine=many, blockSize=1 << 16)
    assert S.readBlockStreams(streams, engine=reader) == [(p, None) for p in payloads]


@pytest.mark.skipif(sc.LZ4_CLI is None, reason="no lz4 command line on this machine")
def test_the_lz4_command_line_reads_the_frames(S, ref, O, payloads):
    many = wm.oracle_many_engine(S, ref, O)
    B = S.FLG.Bits
    for bits in ((B.BLOCK_INDEPENDENCE,), (B.BLOCK_INDEPENDENCE, B.BLOCK_CHECKSUM, B.CONTENT_CHECKSUM, B.CONTENT_SIZE)):
        frames = S.writeFrames(payloads, engine=many, blockSize=S.BLOCKSIZE.SIZE_64KB, bits=bits)
        assert sc.cli(["-d"], b"".join(frames)) == b"".join(payloads)          # concatenated frames, as the CLI reads them
        assert sc.cli(["-d"], frames[-3]) == payloads[-3]
