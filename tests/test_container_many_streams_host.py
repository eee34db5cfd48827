"""streams.readFrames / readBlockStreams on the CPU: the rounds over many readers, with the oracle-backed engine standing in for the
device (streams_common.OracleDeviceEngine has no many-call, so every round's requests are served one by one: the rounds, the hand-over
of requests and results and the readers' own header, end-mark and error code are what runs here; tests/test_gpu_container_many.py
runs the same items through lz4hip_container_decode_many).  Per item the result is the sequential reader's: the same bytes, the same
exception class and message."""
import importlib

import pytest

import container_many_common as cm
import streams_common as sc


@pytest.fixture(scope="module")
def S(amd):
    return importlib.import_module("lz4-java_amd.streams")


@pytest.fixture(scope="module")
def items(ref, corpus):
    return cm.stream_items(ref, corpus, cm.cases(ref, corpus))


@pytest.mark.parametrize("batch", [2, 64])
def test_read_frames_equals_the_sequential_reader(S, ref, O, items, batch):
    engine = sc.OracleDeviceEngine(ref, O)
    want = [cm.read_sequentially(lambda f: S.LZ4FrameInputStream(f, engine=engine, batchBlocks=batch), it) for it in items[0]]
    calls = engine.calls
    cm.same_reads(S.readFrames(items[0], engine=engine, batchBlocks=batch), want, "frames")
    assert engine.calls - calls == calls                   # the same device requests, request for request
    kinds = {type(e).__name__ + ":" + str(e) for _, e in want if e is not None}
    assert len(kinds) >= 8 and any(e is None and d for d, e in want), kinds


@pytest.mark.parametrize("batch", [2, 256])
def test_read_block_streams_equals_the_sequential_reader(S, ref, O, items, batch):
    engine = sc.OracleDeviceEngine(ref, O)
    want = [cm.read_sequentially(lambda f: S.LZ4BlockInputStream(f, engine=engine, batchBlocks=batch), it) for it in items[1]]
    cm.same_reads(S.readBlockStreams(items[1], engine=engine, batchBlocks=batch), want, "block streams")
    assert {str(e) for _, e in want if e is not None} >= {"Stream is corrupted", "Stream ended prematurely"}


def test_rounds_make_one_many_call_each(S, ref, O, items):
    """an engine WITH the many-call gets one call per round, whatever the number of items"""
    class Counting(sc.OracleDeviceEngine):
        rounds = 0

        def containerDecodeMany(self, kind, bodies, maxBlock, nMax, blockChecksum):
            self.rounds += 1
            return [self.containerDecode(kind, b, m, nMax, c) for b, m, c in zip(bodies, maxBlock, blockChecksum)]
    engine = Counting(ref, O)
    frames = [f for f in items[0] if len(f) > 70000][:4] * 10
    got = S.readFrames(frames, engine=engine, batchBlocks=1)
    plain = sc.OracleDeviceEngine(ref, O)
    cm.same_reads(got, [cm.read_sequentially(lambda f: S.LZ4FrameInputStream(f, engine=plain, batchBlocks=1), it) for it in frames], "rounds")
    assert 0 < engine.rounds <= 12 and engine.calls >= 40 * 2, (engine.rounds, engine.calls)


def test_content_checksums_take_one_hash_batch_per_round(S, ref, O, corpus):
    """frames whose content arrives whole in a round are hashed in ONE xxh32 batch behind it and never touch a streaming hash; a frame
    that takes several rounds keeps the streaming hash; a wrong checksum is the sequential reader's error either way"""
    import struct

    class Counting(sc.OracleDeviceEngine):
        def __init__(self, *a):
            super().__init__(*a)
            self.batches, self.updates = [], 0

        def xxh32(self, buf, off, length, seed=0):
            if len(off) > 1 or (len(off) == 1 and length[0] > 16):      # (not a frame descriptor's hash: 2 or 10 bytes, one at a time)
                self.batches.append(len(off))
            return super().xxh32(buf, off, length, seed)

        def newStreamingHash32(self, seed):
            h, eng = super().newStreamingHash32(seed), self
            inner = h.update

            def update(buf, off, length):
                eng.updates += 1
                inner(buf, off, length)
            h.update = update
            return h
    text = corpus["book1[:200000]"]
    frames = []
    for i in range(30):
        content = text[100 * i:100 * i + 300 + i]
        f = cm.frame_header(ref, i % 2 == 0, True, len(content)) + cm.frame_body(ref, [content], i % 2 == 0)
        frames.append(f + struct.pack("<I", ref.xxh32(content, 0) ^ (1 if i == 7 else 0)))
    frames.append(cm.frame_header(ref, False, True) + cm.frame_body(ref, [], False) + struct.pack("<I", ref.xxh32(b"", 0)))   # no content at all
    plain = sc.OracleDeviceEngine(ref, O)
    want = [cm.read_sequentially(lambda f: S.LZ4FrameInputStream(f, engine=plain), it) for it in frames]
    assert str(want[7][1]) == "Content checksum mismatch" and sum(e is None for _, e in want) == 30
    engine = Counting(ref, O)
    cm.same_reads(S.readFrames(frames, engine=engine), want, "whole")
    assert engine.batches == [31] and engine.updates == 0, (engine.batches, engine.updates)
    # one block per round: no content arrives whole with its end mark (the one-block frame's end mark comes a round later)
    content = text[:65536 + 500]
    two = cm.frame_header(ref, False, True) + cm.frame_body(ref, [content[:65536], content[65536:]], False) + struct.pack("<I", ref.xxh32(content, 0))
    engine = Counting(ref, O)
    cm.same_reads(S.readFrames([two, frames[0]], engine=engine, batchBlocks=1),
                  [cm.read_sequentially(lambda f: S.LZ4FrameInputStream(f, engine=plain, batchBlocks=1), it) for it in (two, frames[0])], "streaming")
    assert engine.updates == 3 and engine.batches == [], (engine.updates, engine.batches)
