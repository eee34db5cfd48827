"""Batched twins of the reference's stream/container classes -- SURVEY.md section 8(f), the callers either side
of the block hot path.  The container logic (headers, flags, checks, error messages) follows the reference
class by class; what changes is the cadence: the reference calls `compressor.compress` /
`decompressor.decompress` once per block (LZ4FrameOutputStream.java:199-235, LZ4BlockOutputStream.java:203-227,
LZ4FrameInputStream.java:258-322, LZ4BlockInputStream.java:191-264), these classes queue `batchBlocks`
independent blocks and hand them to ONE `LZ4HIPBatch` launch (and one xxh32 launch for the per-block checksums).

    LZ4FrameOutputStream / LZ4FrameInputStream     LZ4 Frame format v1.5.1 (magic 0x184D2204), interoperable with
                                                   the `lz4` CLI and the reference's classes of the same name
    LZ4BlockOutputStream / LZ4BlockInputStream     lz4-java's own "LZ4Block" container (21-byte block headers)
    LZ4CompressorWithLength / LZ4DecompressorWithLength   4-byte little-endian length prefix

Every data byte is compressed, decompressed and hashed by liblz4hip through `engine` (default: the GPU batch
engine); nothing here falls back to a CPU codec.  `engine` is injectable exactly like the reference's
constructors take a compressor/decompressor/checksum -- the CPU test-suite injects an oracle-backed engine to
check the container logic without a GPU.
"""
import io
import struct

from . import CompressStreams, LZ4Exception, LZ4HIPBatch, LZ4HIPError, maxCompressedLength

_U32 = struct.Struct("<I")
_I32 = struct.Struct("<i")
_U64 = struct.Struct("<Q")


class IOException(IOError):
    """java.io.IOException as thrown by the reference streams"""


class EOFException(IOException):
    pass


class HIPEngine:
    """the batch engine the streams drive: fast or HC compressor + both decompressors + xxh32"""

    def __init__(self, hcLevel=None):
        self.hcLevel = hcLevel

    def compress(self, src, srcOff, srcLen, dst, dstOff, dstCap):
        if self.hcLevel is None:
            return LZ4HIPBatch.compress(src, srcOff, srcLen, dst, dstOff, dstCap)
        return LZ4HIPBatch.compressHC(src, srcOff, srcLen, dst, dstOff, dstCap, self.hcLevel)

    decompressSafe = staticmethod(LZ4HIPBatch.decompressSafe)
    decompressSafeChain = staticmethod(LZ4HIPBatch.decompressSafeChain)   # linked blocks: LZ4FrameInputStream(linkedBlocks=True)
    compressFastChain = staticmethod(LZ4HIPBatch.compressFastChain)       # linked blocks: LZ4FrameOutputStream(linkedBlocks=True)
    compressHCChain = staticmethod(LZ4HIPBatch.compressHCChain)           # linked blocks at an HC level: LZ4FrameOutputStream(linkedBlocks=True, level=N)
    newCompressStreams = staticmethod(CompressStreams)                    # a frame's own resident stream: LZ4FrameOutputStream(linkedBlocks=True, streamState=True)
    decompressFast = staticmethod(LZ4HIPBatch.decompressFast)
    xxh32 = staticmethod(LZ4HIPBatch.xxh32)

    def containerBlocks(self, kind, data, blockSize, blockChecksum=False):
        """round 3: the container bytes of a batch of blocks are laid out on the device behind the compress launch (raw fallback,
        size scan, headers, payload compaction, checksums) -- no host pass between compress and the copy back.  Engines without
        this method (the CPU suite's oracle-backed one) make the writers assemble on the host, byte for byte the same."""
        # (the C ABI reads level 0 as "fast"; an HC engine built with a level < 1 means lz4-java's default HC level, as
        # LZ4Factory.highCompressor(level) does (LZ4Factory.java:263-270: level < 1 -> 9) and as the host-assembly path behaves)
        lv = 0 if self.hcLevel is None else (9 if self.hcLevel < 1 else self.hcLevel)
        return LZ4HIPBatch.containerBlocks(kind, data, blockSize, blockChecksum, lv)

    def containerDecode(self, kind, body, maxBlock, nMax, blockChecksum=False):
        """round 4: the READ side on the device -- size words / 21-byte headers walked, block checksums verified, blocks decoded or
        copied there (lz4hip_container_decode); engines without this method make the readers walk the headers on the host"""
        return LZ4HIPBatch.containerDecode(kind, body, maxBlock, nMax, blockChecksum)

    def containerDecodeMany(self, kind, bodies, maxBlock, nMax, blockChecksum=False):
        """containerDecode for many containers of one kind in ONE call (lz4hip_container_decode_many): lists in, per item the tuple
        containerDecode returns"""
        return LZ4HIPBatch.containerDecodeMany(kind, bodies, maxBlock, nMax, blockChecksum)

    def containerBlocksMany(self, kind, items, blockSizes, blockChecksums=False, gapHead=0, gapTail=0, contentHash=False):
        """containerBlocks for many payloads of one kind in ONE call (lz4hip_container_blocks_many): lists in (or one value for all
        items) -> (dst, off, hashes): item c is dst[off[c]:off[c + 1]], its blocks between gapHead[c] and gapTail[c] zero bytes;
        hashes[c] is the XXH32 (seed 0) of items[c] where contentHash[c] is set"""
        lv = 0 if self.hcLevel is None else (9 if self.hcLevel < 1 else self.hcLevel)
        return LZ4HIPBatch.containerBlocksMany(kind, items, blockSizes, blockChecksums, lv, gapHead, gapTail, contentHash)

    @staticmethod
    def newStreamingHash32(seed):
        """content checksum state (LZ4FrameOutputStream.java:116: `XXHashFactory...newStreamingHash32(0)`)"""
        from . import StreamingXXHash32
        return StreamingXXHash32(seed)


def _compress_batch(engine, data, blockSize):
    """compress data[i*blockSize : +blockSize] for all i in one launch -> (dst, bound, [compressedLength])"""
    n = (len(data) + blockSize - 1) // blockSize
    bound = maxCompressedLength(blockSize)
    dst = bytearray(n * bound)
    offs = [i * blockSize for i in range(n)]
    lens = [min(blockSize, len(data) - o) for o in offs]
    sizes = engine.compress(data, offs, lens, dst, [i * bound for i in range(n)], [bound] * n)
    for s in sizes:
        if s <= 0:
            raise LZ4Exception("maxDestLen is too small")  # LZ4JNICompressor.java:39-41
    return dst, bound, lens, sizes


def _compress_chain(engine, history, data, blockSize, level=None, streams=None, acceleration=1):
    """compress data[i*blockSize : +blockSize] for all i as ONE chain of linked blocks behind `history` -> as _compress_batch; level
    None: the fast chain (LZ4_compress_fast_continue), else the HC chain at that level (LZ4_compress_HC_continue); streams: a set
    whose stream 0 is the frame's and goes on from the batch before (`history` is what it has consumed, at most 64 KB of it);
    acceleration (the fast chain and the stream; 1: the calls as they were): LZ4_compress_fast_continue's last argument"""
    n = (len(data) + blockSize - 1) // blockSize
    bound = maxCompressedLength(blockSize)
    dst = bytearray(n * bound)
    lens = [min(blockSize, len(data) - i * blockSize) for i in range(n)]
    P = len(history)
    kw = {"acceleration": acceleration} if acceleration != 1 else {}
    if streams is not None:
        sizes, _ = streams.compress([0], history + data, [P], lens, [0, n], dst, [i * bound for i in range(n)], [bound] * n, [P], **kw)
    elif level is None:
        sizes, _ = engine.compressFastChain(history + data, [P], lens, [0, n], dst, [i * bound for i in range(n)], [bound] * n, [P], **kw)
    else:
        sizes = engine.compressHCChain(history + data, [P], lens, [0, n], dst, [i * bound for i in range(n)], [bound] * n, [P], level)
    for s in sizes:
        if s <= 0:
            raise LZ4Exception("maxDestLen is too small")
    return dst, bound, lens, list(sizes)


# =================================================================================================
# LZ4 Frame format
# =================================================================================================
class BLOCKSIZE:
    """LZ4FrameOutputStream.java:65-83"""
    SIZE_64KB, SIZE_256KB, SIZE_1MB, SIZE_4MB = 4, 5, 6, 7

    @staticmethod
    def valueOf(indicator):
        if indicator not in (4, 5, 6, 7):
            raise ValueError("Block size must be 4-7. Cannot use value of [%d]" % indicator)
        return indicator

    @staticmethod
    def maximumSize(indicator):  # BD.getBlockMaximumSize, LZ4FrameOutputStream.java:397-399: 2^(2n+8)
        return 1 << (2 * indicator + 8)


class FLG:
    """LZ4FrameOutputStream.java:296-372"""

    class Bits:
        RESERVED_0, RESERVED_1, CONTENT_CHECKSUM, CONTENT_SIZE, BLOCK_CHECKSUM, BLOCK_INDEPENDENCE = 0, 1, 2, 3, 4, 5

    DEFAULT_VERSION = 1
    DEPENDENT_UNSUPPORTED = "Dependent block stream is unsupported (BLOCK_INDEPENDENCE must be set)"

    def __init__(self, version, bits, allowDependent=False):
        self.version = version
        self.bits = bits & 0x3F
        self.allowDependent = allowDependent   # a reader that decodes linked blocks (LZ4FrameInputStream(linkedBlocks=True)): the one way past that check
        self._validate()

    @classmethod
    def of(cls, *bits):
        m = 0
        for b in bits:
            m |= 1 << b
        return cls(cls.DEFAULT_VERSION, m)

    @classmethod
    def fromByte(cls, flg, allowDependent=False):
        return cls((flg >> 6) & 3, flg & 0x3F, allowDependent)

    def toByte(self):
        return self.bits | ((self.version & 3) << 6)

    def isEnabled(self, bit):
        return bool(self.bits >> bit & 1)

    def _validate(self):  # LZ4FrameOutputStream.java:354-367
        if self.isEnabled(self.Bits.RESERVED_0):
            raise RuntimeError("Reserved0 field must be 0")
        if self.isEnabled(self.Bits.RESERVED_1):
            raise RuntimeError("Reserved1 field must be 0")
        if not self.isEnabled(self.Bits.BLOCK_INDEPENDENCE) and not self.allowDependent:
            raise RuntimeError(self.DEPENDENT_UNSUPPORTED)
        if self.version != self.DEFAULT_VERSION:
            raise RuntimeError("Version %d is unsupported" % self.version)


class BD:
    """LZ4FrameOutputStream.java:374-404"""
    RESERVED_MASK = 0x8F

    def __init__(self, blockSizeValue):
        self.blockSizeValue = BLOCKSIZE.valueOf(blockSizeValue)

    @classmethod
    def fromByte(cls, bd):
        if bd & cls.RESERVED_MASK:
            raise RuntimeError("Reserved fields must be 0")
        return cls((bd >> 4) & 7)

    def getBlockMaximumSize(self):
        return BLOCKSIZE.maximumSize(self.blockSizeValue)

    def toByte(self):
        return (self.blockSizeValue & 7) << 4


MAGIC = 0x184D2204
MAGIC_SKIPPABLE_BASE = 0x184D2A50
LZ4_MAX_HEADER_LENGTH = 4 + 1 + 1 + 8 + 1
LZ4_FRAME_INCOMPRESSIBLE_MASK = 0x80000000
PREMATURE_EOS = "Stream ended prematurely"
NOT_SUPPORTED = "Stream unsupported"
BLOCK_HASH_MISMATCH = "Block checksum mismatch"
DESCRIPTOR_HASH_MISMATCH = "Stream frame descriptor corrupted"
CLOSED_STREAM = "The stream is already closed"


class LZ4FrameOutputStream(io.RawIOBase):
    """Twin of lz4/LZ4FrameOutputStream.java.  `out` is any object with write(bytes).  Blocks are queued until
    `batchBlocks` full blocks are buffered (or flush()/close()), then compressed in one launch; the bytes
    written are exactly the reference's for the same input and flags (flush() cuts a short block at the same
    place the reference's flush() does).

    linkedBlocks=True (not in the reference, which writes independent blocks only; the default is False and its bytes are unchanged):
    the frame is written WITHOUT the block-independence flag -- what the `lz4` command line writes by default, and what
    LZ4FrameInputStream(linkedBlocks=True) reads.  Every batch of blocks is ONE chain of linked blocks (engine.compressFastChain:
    LZ4_compress_fast_continue) whose prefix is the last 64 KB this stream wrote of the frame before; a block that does not shrink is
    stored raw and still counts as history for the blocks behind it.  The frame is assembled on the host.  With level=None (the
    default) one frame is one chain on one wavefront at a time: a FORMAT feature (smaller frames for small blocks), not a fast path --
    throughput comes from many chains per launch (LZ4HIPBatch.compressFastChain), not from one stream.

    linkedBlocks=True, level=N: every batch is one HC chain at level N (engine.compressHCChain: LZ4_compress_HC_continue in prefix
    mode, what `lz4 -3` and above write as blocks) behind the last 64 KB written.  A block of an HC chain depends on the 64 KB in
    front of it and on nothing else, so THE FRAME'S BYTES DO NOT DEPEND ON batchBlocks, and the blocks of a batch are parsed at the
    same time, a wavefront each: here a single stream does fill the device, the more blocks a batch holds the better.

    linkedBlocks=True, streamState=True (the fast chain only; the default is False and its bytes are unchanged): the frame is ONE
    compress stream whose table and index position stay on the device from batch to batch (engine.newCompressStreams: a
    CompressStreams set of one), so the blocks are what ONE LZ4_stream_t writes for the whole frame and THE FRAME'S BYTES DO NOT DEPEND
    ON batchBlocks or on flush() calls that fall on block boundaries.  The stream is freed by close().

    linkedBlocks=True, acceleration=N (the fast chain, with or without streamState; the default is 1 and its bytes are unchanged):
    every block is compressed with LZ4_compress_fast_continue(..., N) -- the blocks `lz4 --fast=N` writes (its frames' header flags
    and block sizes are its own).  N is clamped to 1 .. 65537 as liblz4 does.  It has no meaning for an HC level."""

    def __init__(self, out, blockSize=BLOCKSIZE.SIZE_4MB, knownSize=-1, *bits, engine=None, batchBlocks=64, linkedBlocks=False, level=None,
                 streamState=False, acceleration=1):
        super().__init__()
        self.out = out
        self.engine = engine or HIPEngine()
        self.linkedBlocks = linkedBlocks
        self.level = level   # (linkedBlocks) None: the fast chain; else the HC chain's level
        self.history = b""   # (linkedBlocks) the last 64 KB written of the frame
        self._streams = None # (streamState) the frame's resident stream, made at the first batch
        self._streamState = bool(streamState)   # (fixed for the frame: a frame that changed it half way would not be ONE stream's)
        if level is not None and not linkedBlocks:
            raise ValueError("level selects the linked-block compressor: it needs linkedBlocks=True (independent HC blocks: HIPEngine(hcLevel))")
        if streamState and (not linkedBlocks or level is not None):
            raise ValueError("streamState continues the fast chain's stream: it needs linkedBlocks=True and no level")
        self.acceleration = int(acceleration)   # (linkedBlocks, no level) LZ4_compress_fast_continue's last argument
        if self.acceleration != 1 and (not linkedBlocks or level is not None):
            raise ValueError("acceleration is the fast chain's: it needs linkedBlocks=True and no level")
        if streamState and not hasattr(self.engine, "newCompressStreams"):
            raise ValueError("the engine has no resident compress streams")
        if linkedBlocks:
            if not hasattr(self.engine, "compressFastChain" if level is None else "compressHCChain"):
                raise ValueError("the engine cannot compress linked blocks")
            m = 0
            for b in bits:
                if b != FLG.Bits.BLOCK_INDEPENDENCE:
                    m |= 1 << b
            self.flg = FLG(FLG.DEFAULT_VERSION, m, allowDependent=True)
        else:
            if not bits:
                bits = (FLG.Bits.BLOCK_INDEPENDENCE,)
            self.flg = FLG.of(*bits)
        self.bd = BD(blockSize)
        self.maxBlockSize = self.bd.getBlockMaximumSize()
        self.knownSize = knownSize
        self.batchBlocks = max(1, batchBlocks)
        self.buffer = bytearray()
        self.content = self.engine.newStreamingHash32(0) if self.flg.isEnabled(FLG.Bits.CONTENT_CHECKSUM) else None
        self.finished = False
        self._closed = False
        if self.flg.isEnabled(FLG.Bits.CONTENT_SIZE) and knownSize < 0:
            raise ValueError("Known size must be greater than zero in order to use the known size feature")
        self._writeHeader()

    def writable(self):
        return True

    def _writeHeader(self):  # LZ4FrameOutputStream.java:172-190
        head = bytearray(_U32.pack(MAGIC))
        head.append(self.flg.toByte())
        head.append(self.bd.toByte())
        if self.flg.isEnabled(FLG.Bits.CONTENT_SIZE):
            head += _U64.pack(self.knownSize)
        hc = (self.engine.xxh32(bytes(head[4:]), [0], [len(head) - 4], 0)[0] >> 8) & 0xFF
        head.append(hc)
        self.out.write(bytes(head))

    def _ensureNotFinished(self):
        if self.finished or self._closed:
            raise IllegalStateException(CLOSED_STREAM)

    def write(self, b):
        self._ensureNotFinished()
        if isinstance(b, int):
            b = bytes((b & 0xFF,))
        self.buffer += b
        if len(self.buffer) >= self.batchBlocks * self.maxBlockSize:
            full = len(self.buffer) // self.maxBlockSize * self.maxBlockSize
            self._writeBlocks(full)
        return len(b)

    def _writeBlocks(self, nbytes):
        """LZ4FrameOutputStream.writeBlock (:199-235) for every block of buffer[:nbytes] at once"""
        if nbytes == 0:
            return
        data = bytes(self.buffer[:nbytes])
        del self.buffer[:nbytes]
        if self.content is not None:
            self.content.update(data, 0, len(data))  # :211-213: the content checksum streams over the uncompressed bytes
        block_checksum = self.flg.isEnabled(FLG.Bits.BLOCK_CHECKSUM)
        if self.linkedBlocks:                          # one chain behind the last 64 KB written; assembled on the host
            if self._streamState and self._streams is None:
                self._streams = self.engine.newCompressStreams(1)
            dst, bound, lens, sizes = _compress_chain(self.engine, self.history, data, self.maxBlockSize, self.level, self._streams, self.acceleration)
            self.history = (self.history + data)[-65536:]
        elif hasattr(self.engine, "containerBlocks"):   # assembled on the device
            self.out.write(self.engine.containerBlocks(LZ4HIPBatch.FRAME_BLOCKS, data, self.maxBlockSize, block_checksum))
            return
        else:
            dst, bound, lens, sizes = _compress_batch(self.engine, data, self.maxBlockSize)
        outb = bytearray()
        spans = []
        for i, (raw_len, clen) in enumerate(zip(lens, sizes)):
            if clen >= raw_len:  # store uncompressed if compression does not gain
                payload = data[i * self.maxBlockSize: i * self.maxBlockSize + raw_len]
                outb += _U32.pack(raw_len | LZ4_FRAME_INCOMPRESSIBLE_MASK)
            else:
                payload = dst[i * bound: i * bound + clen]
                outb += _U32.pack(clen)
            spans.append((len(outb), len(payload)))
            outb += payload
            if block_checksum:
                outb += b"\0\0\0\0"
        if block_checksum:
            hashes = self.engine.xxh32(outb, [s for s, _ in spans], [n for _, n in spans], 0)
            for (s, n), h in zip(spans, hashes):
                _U32.pack_into(outb, s + n, h)
        self.out.write(bytes(outb))

    def _writeEndMark(self):  # :244-252
        tail = bytearray(_U32.pack(0))
        if self.content is not None:
            tail += _U32.pack(self.content.getValue())
            self.content.close()
        self.out.write(bytes(tail))
        self.finished = True

    def flush(self):  # :279-286: flush() writes the pending (possibly short) block
        if self._closed or self.finished or not hasattr(self, "buffer"):
            return
        self._writeBlocks(len(self.buffer))
        if hasattr(self.out, "flush"):
            self.out.flush()

    def close(self):  # :289-298
        if self._closed:
            return
        if not self.finished:
            self._writeBlocks(len(self.buffer))
            self._writeEndMark()
            if hasattr(self.out, "flush"):
                self.out.flush()
        if self._streams is not None:
            self._streams.close()
            self._streams = None
        self._closed = True
        super().close()


class IllegalStateException(RuntimeError):
    pass


class _Reader:
    """InputStream helpers over any object with read(n)"""

    def __init__(self, inp):
        self.inp = inp
        self.back = b""      # bytes handed back by the device read path (container bytes it did not consume)

    def unread(self, b):
        self.back = bytes(b) + self.back

    def seekable(self):
        try:
            return bool(self.inp.seekable())
        except Exception:
            return False

    def give_back(self):
        """the container ended and the caller goes on reading `inp` itself (readSingleFrame / stopOnEmptyBlock): the bytes the device
        read path took beyond the container's end go back to `inp` -- the reference's readers consume exactly the container
        (LZ4FrameInputStream.java:258-322, LZ4BlockInputStream.java:191-264).  Only seekable inputs get the device path in those modes."""
        if self.back:
            self.inp.seek(-len(self.back), 1)
            self.back = b""

    def read_upto(self, n):
        parts, got = [], 0
        if self.back:
            parts.append(self.back[:n]); got = len(parts[0]); self.back = self.back[got:]
        while got < n:
            c = self.inp.read(n - got)
            if not c:
                break
            parts.append(c)
            got += len(c)
        return b"".join(parts)

    def read_fully(self, n, exc=IOException):
        b = self.read_upto(n)
        if len(b) < n:
            raise exc(PREMATURE_EOS)
        return b


class LZ4FrameInputStream(io.RawIOBase):
    """Twin of lz4/LZ4FrameInputStream.java: concatenated frames, skippable frames, descriptor / block /
    content checksums, content-size check -- same checks, same messages.  Block headers of up to `batchBlocks`
    blocks are parsed ahead, then the block checksums are verified in one xxh32 launch and the compressed
    blocks decoded in one safe-decompress launch.  A defect in block k surfaces when the reader reaches
    block k, after the bytes of blocks < k have been delivered, as in the reference.

    linkedBlocks=True (not in the reference, whose reader refuses such frames; the default refuses them too): a frame without
    BLOCK_INDEPENDENCE -- what the `lz4` command line writes by default -- is read as well.  Its size words are walked on the host,
    `batchBlocks` at a time, and each batch is decoded as ONE chain of linked blocks (engine.decompressSafeChain) whose history is the
    last 64 KB this reader decoded of the frame; stored blocks are part of the chain.  Every check, its order and every message stay as
    they are.  Frames with BLOCK_INDEPENDENCE take the paths above whatever the flag says; an engine without decompressSafeChain keeps
    refusing dependent frames."""

    def __init__(self, inp, readSingleFrame=False, engine=None, batchBlocks=64, hostWalk=False, linkedBlocks=False):
        super().__init__()
        self.linkedBlocks = linkedBlocks
        self.linked = False          # the current frame has no BLOCK_INDEPENDENCE
        self.history = bytearray()   # linked blocks: the last 64 KB decoded of the current frame
        self.hostWalk = hostWalk   # True: headers walked and checksums compared on the host around the batch launches (rounds 1-3)
        self.r = _Reader(inp)
        self.engine = engine or HIPEngine()
        self.readSingleFrame = readSingleFrame
        self.batchBlocks = max(1, batchBlocks)
        self.firstFrameHeaderRead = False
        self.frame_finished = True
        self.flg = self.bd = None
        self.ready = bytearray()  # decoded bytes not yet handed to the reader
        self.pending_exc = None    # raised once `ready` is drained
        self.expectedContentSize = -1
        self.totalContentSize = 0
        self.content = None

    def readable(self):
        return True

    # -- frame level ----------------------------------------------------------------------------
    def _nextFrameInfo(self):  # LZ4FrameInputStream.java:124-160
        while True:
            head = self.r.read_upto(4)
            if len(head) == 0 and self.firstFrameHeaderRead:
                return False  # clean end between frames
            if len(head) < 4:
                raise IOException(PREMATURE_EOS)
            magic = _U32.unpack(head)[0]
            if magic == MAGIC:
                self._readHeader()
                return True
            if magic >> 4 == MAGIC_SKIPPABLE_BASE >> 4:
                skip = _U32.unpack(self.r.read_fully(4))[0]
                self.r.read_fully(skip)
                self.firstFrameHeaderRead = True
            else:
                raise IOException(NOT_SUPPORTED)

    def _readHeader(self):  # :180-224
        fb = self.r.read_fully(2)
        header = bytearray(fb)
        self.flg = FLG.fromByte(fb[0], allowDependent=self.linkedBlocks)
        self.linked = not self.flg.isEnabled(FLG.Bits.BLOCK_INDEPENDENCE)
        if self.linked and not hasattr(self.engine, "decompressSafeChain"):
            raise RuntimeError(FLG.DEPENDENT_UNSUPPORTED)
        self.history = bytearray()
        self.bd = BD.fromByte(fb[1])
        if self.flg.isEnabled(FLG.Bits.CONTENT_SIZE):
            cs = self.r.read_fully(8)
            self.expectedContentSize = _U64.unpack(cs)[0]
            header += cs
        self.totalContentSize = 0
        h = (self.engine.xxh32(bytes(header), [0], [len(header)], 0)[0] >> 8) & 0xFF
        expected = self.r.read_fully(1)[0]
        if h != expected:
            raise IOException(DESCRIPTOR_HASH_MISMATCH)
        self.maxBlockSize = self.bd.getBlockMaximumSize()
        if self.content is not None:
            self.content.close()
        self.content = self.engine.newStreamingHash32(0) if self.flg.isEnabled(FLG.Bits.CONTENT_CHECKSUM) else None
        self.firstFrameHeaderRead = True
        self.frame_finished = False

    # -- block level ----------------------------------------------------------------------------
    def _readBlocksDevice(self):
        """the same on the device (engine.containerDecode): one chunk of container bytes goes over, the decoded blocks and a stop
        reason come back; what the device did not consume is handed back to the reader.  Same checks in the same order, same
        messages; a defect in block k surfaces after the bytes of the blocks before it."""
        req = self._deviceRequest()
        self._deviceResult(req, self.engine.containerDecode(*req[0]))

    def _deviceRequest(self):
        """the first half of _readBlocksDevice: the next chunk of the frame's body as containerDecode's arguments -> (arguments, at_eof).
        readFrames hands the requests of many readers to ONE containerDecodeMany and gives each its result (_deviceResult)"""
        block_checksum = self.flg.isEnabled(FLG.Bits.BLOCK_CHECKSUM)
        want = self.batchBlocks * (self.maxBlockSize + 8) + 4
        chunk = self.r.read_upto(want)
        return (LZ4HIPBatch.FRAME_BLOCKS, chunk, self.maxBlockSize, self.batchBlocks, block_checksum), len(chunk) < want

    def _deviceResult(self, req, result, whole=None):
        """the second half: what containerDecode returned for the request.  whole (a list, readFrames): a frame whose content checksum
        is due and whose WHOLE content is this result does not hash it; (reader, content) is appended, and the caller ends the frame
        with the value of its one xxh32 batch (_finishWhole)"""
        B = LZ4HIPBatch
        (_, chunk, _, _, _), at_eof = req
        decoded, sizes, consumed, why, code = result
        rest = chunk[consumed:]
        batched = whole is not None and self.content is not None and why == B.CR_END and self.totalContentSize == 0
        if decoded:
            first = len(self.ready)
            self.ready += decoded
            self.totalContentSize += len(decoded)
            if self.content is not None and not batched:  # one update per batch of decoded blocks
                self.content.update(self.ready, first, len(decoded))
        self.r.unread(rest)
        if batched:
            whole.append((self, decoded))
            return
        if why == B.CR_END:
            self._endMark()
        elif why == B.CR_BLOCK_TOO_BIG:
            self.r.read_upto(4)
            self.pending_exc = IOException("Block size %s exceeded max: %s" % (_U32.unpack(rest[:4])[0] & ~LZ4_FRAME_INCOMPRESSIBLE_MASK & 0xFFFFFFFF, self.maxBlockSize))
        elif why == B.CR_BLOCK_CHECKSUM:
            self.pending_exc = IOException(BLOCK_HASH_MISMATCH)
        elif why == B.CR_DECODE:  # LZ4JNISafeDecompressor.java:39-41, wrapped in IOException (:307-311)
            self.pending_exc = IOException(LZ4Exception("Error decoding offset %d of input buffer" % (-code)))
        elif why in (B.CR_TRUNCATED, B.CR_MORE) and at_eof:
            self.r.read_upto(len(rest))
            self.pending_exc = IOException(PREMATURE_EOS)
        # (CR_MORE / CR_SLOTS / a chunk that ended inside a block: the next call goes on from the bytes handed back)
        if self.readSingleFrame and self.frame_finished:
            self.r.give_back()

    _deviceDeliver = _deviceResult   # (what _read_many hands a reader for its request of the round)

    def _finishWhole(self, contentHash):
        """the end mark of a frame whose content was hashed by the caller (_deviceResult's `whole`)"""
        self._endMark(contentHash)
        if self.readSingleFrame and self.frame_finished:
            self.r.give_back()

    def _endMark(self, contentHash=None):
        """behind the end mark (LZ4FrameInputStream.java:264-276): content checksum, content size.  contentHash: the content's XXH32
        where the caller has it; None: the streaming hash's"""
        try:
            if self.flg.isEnabled(FLG.Bits.CONTENT_CHECKSUM):
                stored = _U32.unpack(self.r.read_fully(4))[0]
                if stored != (self.content.getValue() if contentHash is None else contentHash):
                    raise IOException("Content checksum mismatch")
            if self.flg.isEnabled(FLG.Bits.CONTENT_SIZE) and self.expectedContentSize != self.totalContentSize:
                raise IOException("Size check mismatch")
        except IOException as e:
            self.pending_exc = e
            return
        self.frame_finished = True

    def _readBlocks(self, defer=None):
        """LZ4FrameInputStream.readBlock (:258-322) for up to batchBlocks blocks.  defer (a list): a device request is not run but
        appended to it, for the caller to run with other readers' (readFrames)"""
        # (the device path takes a whole chunk of container bytes from `inp`: with readSingleFrame the caller reads on behind the
        # frame, so it needs an input it can hand the surplus back to -- round-4 advisor; a pipe or socket gets the host walk, which
        # consumes exactly the frame and never waits for bytes beyond it)
        if not self.linked and not self.hostWalk and hasattr(self.engine, "containerDecode") and (not self.readSingleFrame or self.r.seekable()):
            if defer is not None:
                defer.append(self._deviceRequest())
            else:
                self._readBlocksDevice()
            return
        blocks = []  # (compressed?, payload, stored checksum | None)
        end_mark = False
        exc = None
        block_checksum = self.flg.isEnabled(FLG.Bits.BLOCK_CHECKSUM)
        while len(blocks) < self.batchBlocks:
            try:
                word = _U32.unpack(self.r.read_fully(4))[0]
                compressed = (word & LZ4_FRAME_INCOMPRESSIBLE_MASK) == 0
                size = word & ~LZ4_FRAME_INCOMPRESSIBLE_MASK & 0xFFFFFFFF
                if size == 0:
                    end_mark = True
                    break
                if size > self.maxBlockSize:
                    raise IOException("Block size %s exceeded max: %s" % (size, self.maxBlockSize))
                payload = self.r.read_fully(size)
                stored = _U32.unpack(self.r.read_fully(4))[0] if block_checksum else None
                blocks.append((compressed, payload, stored))
            except IOException as e:
                exc = e
                break
        n = len(blocks)
        if n:
            src = b"".join(p for _, p, _ in blocks)
            offs, o = [], 0
            for _, p, _ in blocks:
                offs.append(o)
                o += len(p)
            lens = [len(p) for _, p, _ in blocks]
            bad = n
            bad_exc = None
            if block_checksum:
                hashes = self.engine.xxh32(src, offs, lens, 0)
                for i, (h, (_, _, stored)) in enumerate(zip(hashes, blocks)):
                    if h != stored:
                        bad, bad_exc = i, IOException(BLOCK_HASH_MISMATCH)
                        break
            if self.linked:
                # one chain: the blocks decode back to back behind the history; a stored block is copied by the same call
                hist = len(self.history)
                dst = bytearray(hist + bad * self.maxBlockSize)
                dst[:hist] = self.history
                res, done = self.engine.decompressSafeChain(src, offs[:bad], lens[:bad], [self.maxBlockSize] * bad, [0, bad], dst, [hist],
                                                            [bad * self.maxBlockSize], [hist], [not c for c, _, _ in blocks[:bad]])
                at = hist
                for i in range(bad):
                    if res[i] < 0:  # LZ4JNISafeDecompressor.java:39-41, wrapped in IOException (:307-311)
                        bad_exc = IOException(LZ4Exception("Error decoding offset %d of input buffer" % (-res[i])))
                        break
                    at += res[i]
                first = len(self.ready)
                self.ready += dst[hist:at]
                self.totalContentSize += at - hist
                self.history = dst[max(at - 65536, 0):at]
                if self.content is not None and at > hist:
                    self.content.update(self.ready, first, at - hist)
                if bad_exc is not None:
                    self.pending_exc = bad_exc
                    return
                if exc is not None:
                    self.pending_exc = exc
                    return
                if end_mark:
                    self._endMark()
                return
            cidx = [i for i in range(bad) if blocks[i][0]]
            outs = [None] * bad
            if cidx:
                dst = bytearray(len(cidx) * self.maxBlockSize)
                res = self.engine.decompressSafe(src, [offs[i] for i in cidx], [lens[i] for i in cidx], dst,
                                                 [k * self.maxBlockSize for k in range(len(cidx))],
                                                 [self.maxBlockSize] * len(cidx))
                for k, i in enumerate(cidx):
                    if res[k] < 0:  # LZ4JNISafeDecompressor.java:39-41, wrapped in IOException (:307-311)
                        bad, bad_exc = i, IOException(LZ4Exception("Error decoding offset %d of input buffer" % (-res[k])))
                        break
                    outs[i] = dst[k * self.maxBlockSize: k * self.maxBlockSize + res[k]]
            first = len(self.ready)
            for i in range(bad):
                piece = outs[i] if blocks[i][0] else blocks[i][1]
                self.ready += piece
                self.totalContentSize += len(piece)
            if self.content is not None and len(self.ready) > first:  # one update per batch of decoded blocks
                self.content.update(self.ready, first, len(self.ready) - first)
            if bad_exc is not None:
                self.pending_exc = bad_exc
                return
        if exc is not None:
            self.pending_exc = exc
            return
        if end_mark:
            self._endMark()

    def _fill(self, defer=None):
        """False at end of stream.  defer (a list): None is returned once a device request waits in it (_readBlocks)"""
        while not self.ready:
            if self.pending_exc is not None:
                e, self.pending_exc = self.pending_exc, None
                raise e
            if not self.firstFrameHeaderRead or self.frame_finished:
                if self.firstFrameHeaderRead and self.frame_finished and self.readSingleFrame and self.flg is not None:
                    return False
                if not self._nextFrameInfo():
                    return False
                if self.frame_finished:  # only skippable frames so far
                    continue
            self._readBlocks(defer)
            if defer:
                return None
        return True

    def read(self, size=-1):
        if size is None or size < 0:
            return self.readall()
        if size == 0:
            return b""
        if not self._fill():
            return b""
        out = bytes(self.ready[:size])
        del self.ready[:size]
        return out

    def readall(self):
        parts = []
        while self._fill():
            parts.append(bytes(self.ready))
            self.ready.clear()
        return b"".join(parts)

    def readinto(self, b):
        data = self.read(len(b))
        b[: len(data)] = data
        return len(data)

    def skip(self, n):  # LZ4FrameInputStream.java:361-379: at most what is decoded and waiting (here: up to one batch of blocks)
        if n <= 0 or not self._fill():
            return 0
        k = min(n, len(self.ready))
        del self.ready[:k]
        return k

    def available(self):  # :382-384
        return len(self.ready)

    def markSupported(self):  # :402-404
        return False

    def mark(self, readlimit):  # :392-394
        raise NotImplementedError("mark not supported")

    def reset(self):  # :397-399
        raise NotImplementedError("reset not supported")

    def getExpectedContentSize(self):  # :375-383
        if not self.firstFrameHeaderRead:
            self._fill()
        return self.expectedContentSize

    def isExpectedContentSizeDefined(self):
        return self.getExpectedContentSize() >= 0


# =================================================================================================
# lz4-java "LZ4Block" container
# =================================================================================================
BLOCK_MAGIC = b"LZ4Block"
MAGIC_LENGTH = len(BLOCK_MAGIC)
HEADER_LENGTH = MAGIC_LENGTH + 1 + 4 + 4 + 4  # LZ4BlockOutputStream.java:42-47
COMPRESSION_LEVEL_BASE = 10
MIN_BLOCK_SIZE = 64
MAX_BLOCK_SIZE = 1 << (COMPRESSION_LEVEL_BASE + 0x0F)
COMPRESSION_METHOD_RAW = 0x10
COMPRESSION_METHOD_LZ4 = 0x20
DEFAULT_SEED = 0x9747B28C
_CHECK_MASK = 0x0FFFFFFF  # StreamingXXHash32.asChecksum keeps 28 bits (StreamingXXHash32.java:101-107)


def _compressionLevel(blockSize):  # LZ4BlockOutputStream.java:57-69
    if blockSize < MIN_BLOCK_SIZE:
        raise ValueError("blockSize must be >= %d, got %d" % (MIN_BLOCK_SIZE, blockSize))
    if blockSize > MAX_BLOCK_SIZE:
        raise ValueError("blockSize must be <= %d, got %d" % (MAX_BLOCK_SIZE, blockSize))
    level = (blockSize - 1).bit_length()  # ceil(log2)
    return max(0, level - COMPRESSION_LEVEL_BASE)


def _user_checks(checksum, pieces):
    """per-block values of a caller-supplied java.util.zip.Checksum-like object (reset / update / getValue), as the reference
    computes them: `checksum.reset(); checksum.update(block); (int) checksum.getValue()` (LZ4BlockOutputStream.java:207-209)"""
    out = []
    for piece in pieces:
        checksum.reset()
        checksum.update(piece, 0, len(piece))
        out.append(checksum.getValue() & 0xFFFFFFFF)
    return out


class LZ4BlockOutputStream(io.RawIOBase):
    """Twin of lz4/LZ4BlockOutputStream.java.  checksum=None is the reference's default (XXH32, seed 0x9747b28c, 28 bits:
    LZ4BlockOutputStream.java:125), computed for all blocks of a batch in one launch; any object with reset() / update(buf, off,
    len) / getValue() -- the java.util.zip.Checksum contract of the 5-argument constructor (:96-101), e.g. an Adler32 or CRC32
    adapter -- is used per block on the host, as the reference does."""

    def __init__(self, out, blockSize=1 << 16, engine=None, syncFlush=False, batchBlocks=256, checksum=None):
        super().__init__()
        self.checksum = checksum
        self.out = out
        self.blockSize = blockSize
        self.compressionLevel = _compressionLevel(blockSize)
        self.engine = engine or HIPEngine()
        self.syncFlush = syncFlush
        self.batchBlocks = max(1, batchBlocks)
        self.buffer = bytearray()
        self.finished = False
        self._closed = False

    def writable(self):
        return True

    def _ensureNotFinished(self):
        if self.finished:
            raise IllegalStateException("This stream is already closed")

    def write(self, b):
        self._ensureNotFinished()
        if isinstance(b, int):
            b = bytes((b & 0xFF,))
        self.buffer += b
        if len(self.buffer) >= self.batchBlocks * self.blockSize:
            self._flushBlocks(len(self.buffer) // self.blockSize * self.blockSize)
        return len(b)

    def _flushBlocks(self, nbytes):
        """flushBufferedData (:203-227) for every block of buffer[:nbytes] at once"""
        if nbytes == 0:
            return
        data = bytes(self.buffer[:nbytes])
        del self.buffer[:nbytes]
        if self.checksum is None and hasattr(self.engine, "containerBlocks"):   # assembled on the device (default XXH32 checksum)
            self.out.write(self.engine.containerBlocks(LZ4HIPBatch.LZ4BLOCK_BLOCKS, data, self.blockSize))
            return
        dst, bound, lens, sizes = _compress_batch(self.engine, data, self.blockSize)
        if self.checksum is None:
            checks = [c & _CHECK_MASK for c in self.engine.xxh32(data, [i * self.blockSize for i in range(len(lens))], lens, DEFAULT_SEED)]
        else:
            checks = _user_checks(self.checksum, [data[i * self.blockSize: i * self.blockSize + n] for i, n in enumerate(lens)])
        outb = bytearray()
        for i, (raw_len, clen, check) in enumerate(zip(lens, sizes, checks)):
            if clen >= raw_len:
                method, clen = COMPRESSION_METHOD_RAW, raw_len
                payload = data[i * self.blockSize: i * self.blockSize + raw_len]
            else:
                method = COMPRESSION_METHOD_LZ4
                payload = dst[i * bound: i * bound + clen]
            outb += BLOCK_MAGIC
            outb.append(method | self.compressionLevel)
            outb += _U32.pack(clen) + _U32.pack(raw_len) + _U32.pack(check)
            outb += payload
        self.out.write(bytes(outb))

    def flush(self):  # :241-248
        if self._closed or not hasattr(self, "buffer"):
            return
        if self.syncFlush and not self.finished:
            self._flushBlocks(len(self.buffer))
        if hasattr(self.out, "flush"):
            self.out.flush()

    def finish(self):  # :256-268
        self._ensureNotFinished()
        self._flushBlocks(len(self.buffer))
        self.out.write(BLOCK_MAGIC + bytes((COMPRESSION_METHOD_RAW | self.compressionLevel,)) + b"\0" * 12)
        self.finished = True
        if hasattr(self.out, "flush"):
            self.out.flush()

    def close(self):
        if self._closed:
            return
        if not self.finished:
            self.finish()
        self._closed = True
        super().close()


class LZ4BlockInputStream(io.RawIOBase):
    """Twin of lz4/LZ4BlockInputStream.java (fast decompressor + default checksum).  Headers of up to
    `batchBlocks` blocks are parsed ahead; LZ4 blocks are decoded in one decompress_fast launch and every
    block's checksum verified in one xxh32 launch."""

    CORRUPTED = "Stream is corrupted"

    def __init__(self, inp, stopOnEmptyBlock=True, engine=None, batchBlocks=256, checksum=None, hostWalk=False):
        super().__init__()
        self.hostWalk = hostWalk   # True: headers walked and checksums compared on the host around the batch launches (rounds 1-3)
        self.checksum = checksum   # None: the default XXH32 (batched); else a Checksum-like object (LZ4BlockInputStream.java:71-76)
        self.r = _Reader(inp)
        self.engine = engine or HIPEngine()
        self.stopOnEmptyBlock = stopOnEmptyBlock
        self.batchBlocks = max(1, batchBlocks)
        self.ready = bytearray()
        self.pending_exc = None
        self.finished = False

    def readable(self):
        return True

    def _refillDevice(self):
        """LZ4BlockInputStream.refill for a run of blocks on the device (engine.containerDecode): headers walked with the reference's
        rules, LZ4 blocks through the fast decoder (its return value must be the header's compressed length), raw ones copied, the
        checksums of the decoded bytes compared -- every defect is "Stream is corrupted", delivered after the blocks before it.
        False: this run is for the host path (a block bigger than the first header announced)."""
        req = self._deviceRequest()
        return req is not None and self._deviceResult(req, self.engine.containerDecode(*req[0]))

    def _deviceRequest(self):
        """the first half of _refillDevice: the next chunk of the stream as containerDecode's arguments -> (arguments, at_eof), or None:
        this run is for the host path.  readBlockStreams hands the requests of many readers to ONE containerDecodeMany and gives each
        its result (_deviceResult)"""
        head = self.r.read_upto(HEADER_LENGTH)
        self.r.unread(head)
        if len(head) < HEADER_LENGTH or head[:MAGIC_LENGTH] != BLOCK_MAGIC:
            return None   # (the host path produces the reference's exception / end of stream)
        maxBlock = 1 << (COMPRESSION_LEVEL_BASE + (head[MAGIC_LENGTH] & 0x0F))
        want = self.batchBlocks * (maxBlock + HEADER_LENGTH) + HEADER_LENGTH
        chunk = self.r.read_upto(want)
        return (LZ4HIPBatch.LZ4BLOCK_BLOCKS, chunk, maxBlock, self.batchBlocks, False), len(chunk) < want

    def _deviceResult(self, req, result):
        """the second half: what containerDecode returned for the request.  False: this run is for the host path"""
        B = LZ4HIPBatch
        (_, chunk, _, _, _), at_eof = req
        decoded, sizes, consumed, why, code = result
        if why == B.CR_BLOCK_TOO_BIG:
            self.r.unread(chunk)
            return False
        if consumed == 0 and not decoded and why in (B.CR_TRUNCATED, B.CR_MORE) and not at_eof:
            # no progress and more input to come: the first header announces a payload longer than this chunk (compressedLen is not
            # bounded by the block size: one flipped bit is enough).  The host path reads exactly what the header says and raises
            # the reference's exception (LZ4BlockInputStream.java:236-253); asking the device again with the same bytes would
            # never end (round-4 advisor, high)
            self.r.unread(chunk)
            return False
        rest = chunk[consumed:]
        self.ready += decoded
        self.r.unread(rest)
        if why == B.CR_END:
            if self.stopOnEmptyBlock:
                self.finished = True
        elif why == B.CR_CORRUPT:
            self.pending_exc = IOException(self.CORRUPTED)
        elif why in (B.CR_TRUNCATED, B.CR_MORE) and at_eof:
            self.r.read_upto(len(rest))
            if len(rest) < HEADER_LENGTH and not self.stopOnEmptyBlock:
                self.finished = True                      # (:192-199: the stream may end at -- or inside -- a header)
            else:
                self.pending_exc = EOFException(PREMATURE_EOS)
        return True

    def _refill(self, defer=None):  # LZ4BlockInputStream.java:191-264, for up to batchBlocks blocks
        """defer (a list): a device request is not run but appended to it, for the caller to run with other readers' (readBlockStreams),
        which then calls _deviceDone"""
        # (stopOnEmptyBlock: the caller reads on behind the empty block, so the device path -- which takes whole chunks from `inp` --
        # needs an input it can hand the surplus back to; see LZ4FrameInputStream._readBlocks)
        if (self.checksum is None and not self.hostWalk and hasattr(self.engine, "containerDecode")
                and (not self.stopOnEmptyBlock or self.r.seekable())):
            if defer is not None:
                req = self._deviceRequest()
                if req is not None:
                    defer.append(req)
                    return
            elif self._refillDevice():
                self._deviceDone()
                return
        self._refillHost()

    def _deviceDone(self):
        """behind a device run that delivered (_deviceResult said True)"""
        if self.stopOnEmptyBlock and self.finished:
            self.r.give_back()

    def _refillHost(self):
        """the headers walked and the checksums compared on the host around the batch launches"""
        blocks = []  # (method, payload, originalLen, check)
        exc = None
        finished = False
        while len(blocks) < self.batchBlocks:
            head = self.r.read_upto(HEADER_LENGTH)
            if len(head) < HEADER_LENGTH:
                if not self.stopOnEmptyBlock:
                    finished = True
                else:
                    exc = EOFException(PREMATURE_EOS)
                break
            try:
                if head[:MAGIC_LENGTH] != BLOCK_MAGIC:
                    raise IOException(self.CORRUPTED)
                token = head[MAGIC_LENGTH]
                method = token & 0xF0
                level = COMPRESSION_LEVEL_BASE + (token & 0x0F)
                if method not in (COMPRESSION_METHOD_RAW, COMPRESSION_METHOD_LZ4):
                    raise IOException(self.CORRUPTED)
                clen, olen, check = struct.unpack_from("<iii", head, MAGIC_LENGTH + 1)
                if (olen > 1 << level or olen < 0 or clen < 0 or (olen == 0 and clen != 0) or (olen != 0 and clen == 0)
                        or (method == COMPRESSION_METHOD_RAW and olen != clen)):
                    raise IOException(self.CORRUPTED)
                if olen == 0 and clen == 0:
                    if check != 0:
                        raise IOException(self.CORRUPTED)
                    if not self.stopOnEmptyBlock:
                        continue
                    finished = True
                    break
                payload = self.r.read_fully(clen, EOFException)
                blocks.append((method, payload, olen, check & 0xFFFFFFFF))
            except IOException as e:
                exc = e
                break
        n = len(blocks)
        if n:
            bad, bad_exc = n, None
            lz = [i for i in range(n) if blocks[i][0] == COMPRESSION_METHOD_LZ4]
            raw = [None] * n
            if lz:
                # decompress_fast reads the source without a length; pad so the bounded kernel has slack
                src = b"".join(blocks[i][1] for i in lz)
                soff, o = [], 0
                for i in lz:
                    soff.append(o)
                    o += len(blocks[i][1])
                doff, o = [], 0
                for i in lz:
                    doff.append(o)
                    o += blocks[i][2]
                dst = bytearray(o)
                res = self.engine.decompressFast(src, soff, [len(blocks[i][1]) for i in lz], dst, doff,
                                                 [blocks[i][2] for i in lz])
                for k, i in enumerate(lz):
                    if res[k] < 0 or res[k] != len(blocks[i][1]):  # :246-253
                        bad, bad_exc = i, IOException(self.CORRUPTED)
                        break
                    raw[i] = bytes(dst[doff[k]: doff[k] + blocks[i][2]])
            for i in range(bad):
                if raw[i] is None:
                    raw[i] = blocks[i][1]
            if bad:
                allb = b"".join(raw[:bad])
                offs, o = [], 0
                for i in range(bad):
                    offs.append(o)
                    o += len(raw[i])
                if self.checksum is None:
                    hashes = [h & _CHECK_MASK for h in self.engine.xxh32(allb, offs, [len(raw[i]) for i in range(bad)], DEFAULT_SEED)]
                else:
                    hashes = _user_checks(self.checksum, raw[:bad])
                for i in range(bad):
                    if hashes[i] != blocks[i][3]:
                        bad, bad_exc = i, IOException(self.CORRUPTED)
                        break
            for i in range(bad):
                self.ready += raw[i]
            if bad_exc is not None:
                self.pending_exc = bad_exc
                return
        if exc is not None:
            self.pending_exc = exc
        elif finished:
            self.finished = True

    def _fill(self, defer=None):
        """defer (a list): None is returned once a device request waits in it (_refill)"""
        while not self.ready:
            if self.pending_exc is not None:
                e, self.pending_exc = self.pending_exc, None
                raise e
            if self.finished:
                return False
            self._refill(defer)
            if defer:
                return None
        return True

    def read(self, size=-1):
        if size is None or size < 0:
            return self.readall()
        if size == 0 or not self._fill():
            return b""
        out = bytes(self.ready[:size])
        del self.ready[:size]
        return out

    def readall(self):
        parts = []
        while self._fill():
            parts.append(bytes(self.ready))
            self.ready.clear()
        return b"".join(parts)

    def readinto(self, b):
        data = self.read(len(b))
        b[: len(data)] = data
        return len(data)

    def skip(self, n):  # LZ4BlockInputStream.java:176-189: at most what is decoded and waiting (here: up to one batch of blocks)
        if n <= 0 or self.finished and not self.ready:
            return 0
        if not self._fill():
            return 0
        k = min(n, len(self.ready))
        del self.ready[:k]
        return k

    def available(self):  # :134-136
        return len(self.ready)

    def markSupported(self):  # :288-290
        return False

    def mark(self, readlimit):  # :294-296: unsupported, silently
        pass

    def reset(self):  # :300-302
        raise IOException("mark/reset not supported")

    def _deviceDeliver(self, req, result, whole=None):
        """what _read_many hands a reader for its request of the round (whole: the frame reader's)"""
        if self._deviceResult(req, result):
            self._deviceDone()
        else:
            self._refillHost()


# =================================================================================================
# many containers at once
# =================================================================================================
def _read_many(readers, engine, kind):
    """The readers -- one per item, each the sequential reader of its item -- driven in ROUNDS: in a round every unfinished reader
    parses what lies in front of its next blocks (frame headers, skippable frames, end marks, content size and checksum: its own
    code) and hands over the rest of its current body as a device request; the requests of all readers go into ONE
    containerDecodeMany, and every reader takes its result as if it had made the call itself.  CR_SLOTS and CR_MORE carry on in the
    next round.  Content checksums: the frames whose content arrived whole in a round are hashed in ONE xxh32 batch behind it; a frame
    that takes several rounds keeps its streaming hash.
    -> per item (data, error): the bytes the reader delivers before it stops, and None or the exception it raises"""
    n = len(readers)
    out, err = [bytearray() for _ in range(n)], [None] * n
    many = getattr(engine, "containerDecodeMany", None)
    live = list(range(n))
    while live:
        waiting = []
        for i in live:
            r, defer = readers[i], []
            try:
                while True:
                    more = r._fill(defer)
                    if more is None:
                        waiting.append((i, defer[0]))
                    if not more:
                        break
                    out[i] += r.ready
                    r.ready.clear()
            except LZ4HIPError:      # (the library failed -- no device, no memory: the call's failure, not an item's result)
                raise
            except Exception as e:   # noqa: BLE001 -- whatever the sequential reader raises is the item's result
                err[i] = e
        if not waiting:
            break
        args = [q[0] for _, q in waiting]
        if many is not None:
            results = many(kind, [a[1] for a in args], [a[2] for a in args], args[0][3], [a[4] for a in args])
        else:                        # (an engine without the many-call: the same requests one by one)
            results = [engine.containerDecode(*a) for a in args]
        live, whole = [], []
        for (i, req), res in zip(waiting, results):
            try:
                readers[i]._deviceDeliver(req, res, whole)
                live.append(i)
            except LZ4HIPError:
                raise
            except Exception as e:   # noqa: BLE001
                err[i] = e
        if whole:                    # one hash launch for the contents that arrived whole in this round
            offs, o = [], 0
            for _, d in whole:
                offs.append(o)
                o += len(d)
            hashes = engine.xxh32(b"".join(bytes(d) for _, d in whole), offs, [len(d) for _, d in whole], 0)
            for (r, _), h in zip(whole, hashes):
                r._finishWhole(h)
    return [(bytes(o), e) for o, e in zip(out, err)]


def readFrames(items, engine=None, batchBlocks=64):
    """Many LZ4 Frame streams read together: for each item (data, error) -- the bytes LZ4FrameInputStream(io.BytesIO(item)) delivers
    before it stops, and None or the exception it raises (same class, same message).  Every round of block reading is one
    containerDecodeMany over all unfinished items (lz4hip_container_decode_many) where the sequential readers make one containerDecode
    each; concatenated and skippable frames, end marks, content size and content checksum are the reader's own code.  Frames with
    linked blocks are not part of the many-call: the reader refuses them, as it does alone."""
    engine = engine or HIPEngine()
    return _read_many([LZ4FrameInputStream(io.BytesIO(bytes(it)), engine=engine, batchBlocks=batchBlocks) for it in items], engine, LZ4HIPBatch.FRAME_BLOCKS)


def readBlockStreams(items, engine=None, batchBlocks=256):
    """Many lz4-java "LZ4Block" streams read together: readFrames' twin over LZ4BlockInputStream(io.BytesIO(item))"""
    engine = engine or HIPEngine()
    return _read_many([LZ4BlockInputStream(io.BytesIO(bytes(it)), engine=engine, batchBlocks=batchBlocks) for it in items], engine, LZ4HIPBatch.LZ4BLOCK_BLOCKS)


def writeFrames(payloads, engine=None, blockSize=BLOCKSIZE.SIZE_4MB, bits=()):
    """Many LZ4 Frames written together: for each payload the complete frame, byte for byte what
    LZ4FrameOutputStream(out, blockSize, len(payload), *bits, engine=engine) writes when the payload is written to it and it is closed
    (bits: FLG.Bits values; with CONTENT_SIZE every frame carries its payload's length).  All payloads' blocks are made by ONE
    containerBlocksMany (lz4hip_container_blocks_many) where the writers make a containerBlocks each; the frame header, the end mark
    and the content checksum -- taken on the device in the same call -- go into the gaps the call leaves around each item's blocks.
    Frames with linked blocks are not part of the many-call.  An engine without containerBlocksMany writes frame by frame."""
    engine = engine or HIPEngine()
    bits = tuple(bits) or (FLG.Bits.BLOCK_INDEPENDENCE,)
    payloads = [bytes(p) if not isinstance(p, (bytes, bytearray)) else p for p in payloads]
    many = getattr(engine, "containerBlocksMany", None)
    if many is None:
        out = []
        for p in payloads:
            sink = io.BytesIO()
            w = LZ4FrameOutputStream(sink, blockSize, len(p) if FLG.Bits.CONTENT_SIZE in bits else -1, *bits, engine=engine)
            w.write(p)
            w.close()
            out.append(sink.getvalue())
        return out
    flg, bd = FLG.of(*bits), BD(blockSize)
    if not payloads:
        return []
    sized, summed = flg.isEnabled(FLG.Bits.CONTENT_SIZE), flg.isEnabled(FLG.Bits.CONTENT_CHECKSUM)
    # the descriptors (LZ4FrameOutputStream._writeHeader): one xxh32 batch over the distinct ones
    desc = [bytes((flg.toByte(), bd.toByte())) + (_U64.pack(len(p)) if sized else b"") for p in payloads]
    distinct = sorted(set(desc))
    offs, at = [], 0
    for d in distinct:
        offs.append(at); at += len(d)
    hc = dict(zip(distinct, engine.xxh32(b"".join(distinct), offs, [len(d) for d in distinct], 0)))
    heads = [_U32.pack(MAGIC) + d + bytes(((hc[d] >> 8) & 0xFF,)) for d in desc]
    n = len(payloads)
    dst, off, hashes = many(LZ4HIPBatch.FRAME_BLOCKS, payloads, [bd.getBlockMaximumSize()] * n, [flg.isEnabled(FLG.Bits.BLOCK_CHECKSUM)] * n,
                            [len(h) for h in heads], [8 if summed else 4] * n, [summed] * n)
    out = []
    for c in range(n):
        item = bytearray(dst[int(off[c]):int(off[c + 1])])
        item[:len(heads[c])] = heads[c]
        if summed:                       # (the four bytes in front of it are the end mark: zeros already)
            _U32.pack_into(item, len(item) - 4, int(hashes[c]))
        out.append(bytes(item))
    return out


def writeBlockStreams(payloads, engine=None, blockSize=1 << 16):
    """Many lz4-java "LZ4Block" streams written together: writeFrames' twin -- for each payload what LZ4BlockOutputStream(out,
    blockSize, engine=engine) writes when the payload is written to it and it is closed (the default checksum); the empty end block
    goes into the gap behind each item's blocks"""
    engine = engine or HIPEngine()
    level = _compressionLevel(blockSize)
    payloads = [bytes(p) if not isinstance(p, (bytes, bytearray)) else p for p in payloads]
    many = getattr(engine, "containerBlocksMany", None)
    if many is None:
        out = []
        for p in payloads:
            sink = io.BytesIO()
            w = LZ4BlockOutputStream(sink, blockSize, engine=engine)
            w.write(p)
            w.close()
            out.append(sink.getvalue())
        return out
    if not payloads:
        return []
    n = len(payloads)
    end = BLOCK_MAGIC + bytes((COMPRESSION_METHOD_RAW | level,))   # (LZ4BlockOutputStream.finish: twelve zero bytes follow)
    dst, off, _ = many(LZ4HIPBatch.LZ4BLOCK_BLOCKS, payloads, [blockSize] * n, [False] * n, [0] * n, [21] * n, [False] * n)
    out = []
    for c in range(n):
        item = bytearray(dst[int(off[c]):int(off[c + 1])])
        item[len(item) - 21:len(item) - 21 + len(end)] = end
        out.append(bytes(item))
    return out


# =================================================================================================
# length-prefixed blocks
# =================================================================================================
class LZ4CompressorWithLength:
    """lz4/LZ4CompressorWithLength.java: 4-byte little-endian decompressed length, then the block.
    compressMany() is the batched form (one launch for a list of buffers)."""

    def __init__(self, compressor=None, engine=None):
        self.compressor = compressor
        self.engine = engine or HIPEngine()

    def maxCompressedLength(self, length):  # :65-67
        return maxCompressedLength(length) + 4

    def compress(self, src, srcOff=0, srcLen=None):  # :76-110
        srcLen = len(src) - srcOff if srcLen is None else srcLen
        if self.compressor is not None:
            body = self.compressor.compress(src, srcOff, srcLen)
            return _I32.pack(srcLen) + body
        return self.compressMany([bytes(src[srcOff: srcOff + srcLen])])[0]

    def compressMany(self, bufs):
        src = b"".join(bufs)
        offs, o = [], 0
        for b in bufs:
            offs.append(o)
            o += len(b)
        caps = [maxCompressedLength(len(b)) for b in bufs]
        doffs, o = [], 0
        for c in caps:
            doffs.append(o)
            o += c
        dst = bytearray(o)
        sizes = self.engine.compress(src, offs, [len(b) for b in bufs], dst, doffs, caps)
        out = []
        for b, d, s in zip(bufs, doffs, sizes):
            if s <= 0:
                raise LZ4Exception("maxDestLen is too small")
            out.append(_I32.pack(len(b)) + bytes(dst[d: d + s]))
        return out


class LZ4DecompressorWithLength:
    """lz4/LZ4DecompressorWithLength.java.  fast=True follows the LZ4FastDecompressor constructor (:84-87: the
    result is the number of source bytes read), fast=False the LZ4SafeDecompressor one (:94-97)."""

    def __init__(self, fast=True, engine=None):
        self.fast = fast
        self.engine = engine or HIPEngine()

    @staticmethod
    def getDecompressedLength(src, srcOff=0):  # :52-54
        return _I32.unpack_from(src, srcOff)[0]

    def decompress(self, src, srcOff=0, srcLen=None):
        srcLen = len(src) - srcOff if srcLen is None else srcLen
        return self.decompressMany([bytes(src[srcOff: srcOff + srcLen])])[0]

    def decompressMany(self, bufs):
        lens = [self.getDecompressedLength(b) for b in bufs]
        for n in lens:
            if n < 0:
                raise ValueError("lengths must be >= 0")
        src = b"".join(bufs)
        soff, o = [], 0
        for b in bufs:
            soff.append(o + 4)
            o += len(b)
        doff, o = [], 0
        for n in lens:
            doff.append(o)
            o += n
        dst = bytearray(o)
        slens = [len(b) - 4 for b in bufs]
        fn = self.engine.decompressFast if self.fast else self.engine.decompressSafe
        res = fn(src, soff, slens, dst, doff, lens)
        out = []
        for i, r in enumerate(res):
            if r < 0:
                raise LZ4Exception("Error decoding offset %d of input buffer" % (4 - r))
            # safe path: LZ4SafeDecompressor.decompress(src, off, len, maxDestLen) trims to the decoded length
            out.append(bytes(dst[doff[i]: doff[i] + (lens[i] if self.fast else r)]))
        return out
