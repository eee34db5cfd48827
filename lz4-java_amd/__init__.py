"""lz4-java_amd -- host-side mirror of lz4-java's plugin interface for the "HIP" family.

The reference is Java; this image has no JDK, so the host side above the C ABI
(``include/lz4hip.h`` / ``liblz4hip.so``) is mirrored here 1:1 for the test-suite and bench (the
Java classes + JNI shim a maintainer would add are in ``java/`` and ``INTEGRATION.md``):

====================================  =========================================================
reference (src/java/net/jpountz/...)  here
====================================  =========================================================
lz4/LZ4Factory.java:91-126,229-291    ``LZ4Factory.hipInstance()`` .fastCompressor() .highCompressor()
                                      .fastDecompressor() .safeDecompressor()
lz4/LZ4Compressor.java:36,59,96-147   ``LZ4Compressor.maxCompressedLength / compress(...)``
lz4/LZ4JNICompressor.java:35-43       ``LZ4HIPCompressor`` (range checks -> native -> LZ4Exception)
lz4/LZ4SafeDecompressor.java:45-135   ``LZ4SafeDecompressor.decompress(...)``
lz4/LZ4FastDecompressor.java:48-121   ``LZ4FastDecompressor.decompress(...)``
lz4/LZ4Exception.java                 ``LZ4Exception``
util/SafeUtils.java:24-42             ``_check_range`` (ArrayIndexOutOfBounds -> IndexError,
                                      IllegalArgument -> ValueError)
xxhash/XXHashFactory.java:80,211,220  ``XXHashFactory.hipInstance().hash32() / hash64()``
xxhash/XXHash32.java:38 / XXHash64    ``XXHash32.hash(buf, off, len, seed)`` / ``XXHash64.hash``
(no equivalent: one block per call)   ``LZ4HIPBatch`` -- many independent blocks per HIP launch
====================================  =========================================================

There is no CPU implementation in this package: every codec call goes through liblz4hip.so and
fails with ``LZ4HIPError`` when the library or a GPU is missing.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (developer A/B builds: LZ4HIP_LIBRARY names another build of the SAME library, e.g. lz4-java_amd/variants/<name>.so of tools/build_variant.sh)
_LIB_PATH = os.environ.get("LZ4HIP_LIBRARY") or os.path.join(_HERE, "liblz4hip.so")
_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)

# every symbol include/lz4hip.h declares (tests check the built library exports all of them)
C_ABI = {
    "lz4hip_init": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "lz4hip_shutdown": (None, []),
    "lz4hip_device_count": (C.c_int, []),
    "lz4hip_last_error": (C.c_char_p, []),
    "lz4hip_version": (C.c_int, []),
    "lz4hip_set_option": (C.c_int, [C.c_char_p, C.c_int]),
    "lz4hip_last_decode_route": (C.c_int, [C.c_int, C.POINTER(C.c_uint32)]),
    "lz4hip_compress_bound": (C.c_int, [C.c_int]),
    "lz4hip_compress_fast_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _u64p, _i32p, _i32p, C.c_uint32]),
    "lz4hip_compress_fast_accel_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _u64p, _i32p, _i32p, C.c_uint32, C.c_int]),
    "lz4hip_compress_dest_size_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _u64p, _i32p, _i32p, _i32p, C.c_uint32]),
    "lz4hip_compress_hc_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _u64p, _i32p, _i32p, C.c_uint32, C.c_int]),
    "lz4hip_compress_hc_dest_size_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _u64p, _i32p, _i32p, _i32p, C.c_uint32, C.c_int]),
    "lz4hip_decompress_safe_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _u64p, _i32p, _i32p, C.c_uint32]),
    "lz4hip_decompress_fast_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _u64p, _i32p, _i32p, C.c_uint32]),
    "lz4hip_decompress_safe_partial_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _u64p, _i32p, _i32p, _i32p, C.c_uint32]),
    "lz4hip_decompressed_size_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, _i32p, _i32p, C.c_uint32]),
    "lz4hip_dict_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "lz4hip_dict_size": (C.c_int, [C.c_void_p]),
    "lz4hip_dict_free": (None, [C.c_void_p]),
    "lz4hip_compress_fast_dict_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _u64p, _i32p, _i32p, C.c_uint32, C.c_void_p]),
    "lz4hip_decompress_safe_dict_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _u64p, _i32p, _i32p, C.c_uint32, C.c_void_p]),
    "lz4hip_compress_hc_dict_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _u64p, _i32p, _i32p, C.c_uint32, C.c_int, C.c_void_p]),
    "lz4hip_decompress_safe_chain_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_void_p, _i32p, _u32p, C.c_void_p, _u64p, _u64p, C.c_void_p, _i32p, _u64p,
                                                     C.c_uint32, C.c_uint32]),
    "lz4hip_decompress_safe_chain_batch_dev": (C.c_int, [C.c_void_p] * 12 + [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]),
    "lz4hip_decompress_safe_stream_batch": (C.c_int, [_u64p, C.c_void_p, _u64p, _i32p, _u32p, C.c_void_p, _u64p, _i32p, _u64p, _u64p, _i32p,
                                                      C.c_uint32, C.c_uint32]),
    "lz4hip_decompress_safe_stream_inorder_batch": (C.c_int, [_u64p, C.c_void_p, _u64p, _i32p, _u32p, C.c_void_p, _u64p, _i32p, _u64p, _u64p, _i32p,
                                                              C.c_uint32, C.c_uint32]),
    "lz4hip_decoder_ring_buffer_size": (C.c_int, [C.c_int]),
    "lz4hip_compress_fast_chain_batch": (C.c_int, [C.c_void_p, _u64p, C.c_void_p, _i32p, _u32p, C.c_void_p, _u64p, _i32p, _i32p, _u64p, C.c_uint32, C.c_uint32]),
    "lz4hip_compress_fast_chain_batch_dev": (C.c_int, [C.c_void_p] * 10 + [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]),
    "lz4hip_compress_fast_chain_accel_batch": (C.c_int, [C.c_void_p, _u64p, C.c_void_p, _i32p, _u32p, C.c_void_p, _u64p, _i32p, _i32p, _u64p, C.c_uint32, C.c_uint32,
                                                         C.c_int]),
    "lz4hip_compress_hc_chain_batch": (C.c_int, [C.c_void_p, _u64p, C.c_void_p, _i32p, _u32p, C.c_void_p, _u64p, _i32p, _i32p, C.c_uint32, C.c_uint32, C.c_int]),
    "lz4hip_compress_hc_stream_batch": (C.c_int, [_u64p, C.c_void_p, _u64p, _i32p, _u32p, C.c_void_p, _u64p, _i32p, _i32p, C.c_uint32, C.c_uint32, C.c_int]),
    "lz4hip_hcstream_load_dict": (C.c_int, [_u64p, C.c_uint64, C.c_uint64]),
    "lz4hip_hcstream_save_dict": (C.c_int, [_u64p, C.c_uint64, C.c_int]),
    "lz4hip_cstreams_create": (C.c_int, [C.c_uint32, C.POINTER(C.c_void_p)]),
    "lz4hip_cstreams_count": (C.c_int, [C.c_void_p]),
    "lz4hip_cstreams_reset": (C.c_int, [C.c_void_p, _u32p, C.c_uint32]),
    "lz4hip_cstreams_consumed": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _u64p, C.c_void_p]),
    "lz4hip_cstreams_free": (None, [C.c_void_p]),
    "lz4hip_compress_fast_stream_batch": (C.c_int, [C.c_void_p, _u32p, C.c_void_p, _u64p, C.c_void_p, _i32p, _u32p, C.c_void_p, _u64p, _i32p, _i32p, _u64p,
                                                    C.c_uint32, C.c_uint32]),
    "lz4hip_compress_fast_stream_ext_batch": (C.c_int, [C.c_void_p, _u32p, C.c_void_p, _u64p, _i32p, _u32p, _u64p, _i32p, _u64p, _u64p, C.c_void_p, _u64p,
                                                        _i32p, _i32p, _u64p, C.c_uint32, C.c_uint32]),
    "lz4hip_compress_fast_stream_accel_batch": (C.c_int, [C.c_void_p, _u32p, C.c_void_p, _u64p, C.c_void_p, _i32p, _u32p, C.c_void_p, _u64p, _i32p, _i32p, _u64p,
                                                          C.c_uint32, C.c_uint32, C.c_int]),
    "lz4hip_compress_fast_stream_ext_accel_batch": (C.c_int, [C.c_void_p, _u32p, C.c_void_p, _u64p, _i32p, _u32p, _u64p, _i32p, _u64p, _u64p, C.c_void_p, _u64p,
                                                              _i32p, _i32p, _u64p, C.c_uint32, C.c_uint32, C.c_int]),
    "lz4hip_xxh32_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_uint32, _u32p, C.c_uint32]),
    "lz4hip_xxh64_batch": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_uint64, _u64p, C.c_uint32]),
    "lz4hip_compress_fast_batch_dev": (C.c_int, [C.c_void_p] * 7 + [C.c_uint32, C.c_int, C.c_void_p]),
    "lz4hip_compress_fast_accel_batch_dev": (C.c_int, [C.c_void_p] * 7 + [C.c_uint32, C.c_int, C.c_int, C.c_void_p]),
    "lz4hip_compress_dest_size_batch_dev": (C.c_int, [C.c_void_p] * 8 + [C.c_uint32, C.c_int, C.c_void_p]),
    "lz4hip_decompress_safe_partial_batch_dev": (C.c_int, [C.c_void_p] * 8 + [C.c_uint32, C.c_int, C.c_void_p]),
    "lz4hip_compress_fast_dict_batch_dev": (C.c_int, [C.c_void_p] * 7 + [C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]),
    "lz4hip_compress_hc_dict_batch_dev": (C.c_int, [C.c_void_p] * 7 + [C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "lz4hip_compress_hc_dict_batch_dev_ws": (C.c_int, [C.c_void_p] * 7 + [C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]),
    "lz4hip_decompress_safe_dict_batch_dev": (C.c_int, [C.c_void_p] * 7 + [C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "lz4hip_compress_hc_batch_dev": (C.c_int, [C.c_void_p] * 7 + [C.c_uint32, C.c_int, C.c_int, C.c_void_p]),
    "lz4hip_compress_hc_dest_size_batch_dev": (C.c_int, [C.c_void_p] * 8 + [C.c_uint32, C.c_int, C.c_int, C.c_void_p]),
    "lz4hip_compress_hc_dest_size_batch_dev_ws": (C.c_int, [C.c_void_p] * 8 + [C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]),
    "lz4hip_hc_workspace_bytes": (C.c_size_t, [C.c_uint64, C.c_uint32, C.c_int]),
    "lz4hip_compress_hc_batch_dev_ws": (C.c_int, [C.c_void_p] * 7 + [C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]),
    "lz4hip_decompress_safe_batch_dev": (C.c_int, [C.c_void_p] * 7 + [C.c_uint32, C.c_int, C.c_void_p]),
    "lz4hip_decompress_fast_batch_dev": (C.c_int, [C.c_void_p] * 7 + [C.c_uint32, C.c_int, C.c_void_p]),
    "lz4hip_decompressed_size_batch_dev": (C.c_int, [C.c_void_p] * 5 + [C.c_uint32, C.c_int, C.c_void_p]),
    "lz4hip_xxh32_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]),
    "lz4hip_xxh64_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]),
    "lz4hip_compress_fast": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "lz4hip_compress_fast_accel": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "lz4hip_compress_dest_size": (C.c_int, [C.c_void_p, _i32p, C.c_void_p, C.c_int]),
    "lz4hip_compress_hc": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "lz4hip_compress_hc_dest_size": (C.c_int, [C.c_void_p, _i32p, C.c_void_p, C.c_int, C.c_int]),
    "lz4hip_decompress_safe": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "lz4hip_decompress_fast": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "lz4hip_decompress_safe_partial": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "lz4hip_compress_fast_dict": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "lz4hip_decompress_safe_dict": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "lz4hip_compress_hc_dict": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "lz4hip_decompressed_size": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "lz4hip_xxh32": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, _u32p]),
    "lz4hip_xxh64": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, _u64p]),
    "lz4hip_xxh32_stream_create": (C.c_int, [C.c_uint32, C.POINTER(C.c_void_p)]),
    "lz4hip_xxh64_stream_create": (C.c_int, [C.c_uint64, C.POINTER(C.c_void_p)]),
    "lz4hip_xxh_stream_reset": (C.c_int, [C.c_void_p, C.c_uint64]),
    "lz4hip_xxh_stream_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "lz4hip_xxh_stream_update_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "lz4hip_xxh32_stream_digest": (C.c_int, [C.c_void_p, _u32p]),
    "lz4hip_xxh64_stream_digest": (C.c_int, [C.c_void_p, _u64p]),
    "lz4hip_xxh_stream_free": (None, [C.c_void_p]),
    "lz4hip_container_workspace_bytes": (C.c_size_t, [C.c_uint64, C.c_uint32, C.c_int]),
    "lz4hip_container_blocks": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, _u64p]),
    "lz4hip_container_blocks_dev": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "lz4hip_container_decode_workspace_bytes": (C.c_size_t, [C.c_uint32]),
    "lz4hip_container_decode_dev": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "lz4hip_container_decode": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "lz4hip_container_decode_bound": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "lz4hip_container_decode_many_bound": (C.c_int, [C.c_int, C.c_void_p, _u64p, _u64p, _u32p, _u8p, C.c_uint32, C.c_uint32, _u32p, _u64p]),
    "lz4hip_container_decode_many": (C.c_int, [C.c_int, C.c_void_p, _u64p, _u64p, _u32p, _u8p, C.c_uint32, C.c_uint32, _u8p, C.c_uint64, _u64p, _u32p,
                                               _i32p, C.c_uint32, _u64p]),
    "lz4hip_container_blocks_many_bound": (C.c_int, [C.c_int, _u64p, _u32p, _u8p, _u32p, _u32p, C.c_uint32, _u32p, _u64p]),
    "lz4hip_container_blocks_many": (C.c_int, [C.c_int, C.c_int, C.c_void_p, _u64p, _u64p, _u32p, _u8p, _u32p, _u32p, C.c_uint32, _u8p, C.c_uint64, _u64p,
                                               _u32p]),
    "lz4hip_gen_blocks_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.c_int, C.c_void_p]),
}

_INT32_MIN = -(2 ** 31)


class LZ4Exception(Exception):
    """lz4/LZ4Exception.java -- codec-level failure (dest too small, malformed input)."""


class LZ4HIPError(RuntimeError):
    """Library-level failure: liblz4hip.so missing, no GPU, HIP error.  Never a silent fallback."""


class ReadOnlyBufferException(TypeError):
    """java.nio.ReadOnlyBufferException analogue (ByteBufferUtils.java:99-103)."""


_lib = None


def lib():
    """The loaded C-ABI library (raises LZ4HIPError if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise LZ4HIPError("%s not built: run lz4-java_amd/build.sh (or __graft_entry__.build())" % _LIB_PATH)
        try:
            import torch  # noqa: F401  -- share PyTorch's HIP runtime (same SONAME) when it is there
        except Exception:
            pass
        l = C.CDLL(_LIB_PATH)
        for name, (res, args) in C_ABI.items():
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        if hasattr(l, "lz4hip_dbg_compress_fast_profile_dev"):   # developer builds only (-DLZ4HIP_DEV_TOOLS)
            l.lz4hip_dbg_compress_fast_profile_dev.restype = C.c_int
            l.lz4hip_dbg_compress_fast_profile_dev.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
        _lib = l
    return _lib


def _chk(rc):
    if rc != 0:
        raise LZ4HIPError("liblz4hip status %d: %s" % (rc, (lib().lz4hip_last_error() or b"").decode()))


def _single(ret):
    if ret < _INT32_MIN + 64:
        raise LZ4HIPError("liblz4hip status %d: %s" % (-(ret - _INT32_MIN), (lib().lz4hip_last_error() or b"").decode()))
    return ret


def _check_length(n):  # SafeUtils.java:38-42
    if n < 0:
        raise ValueError("lengths must be >= 0")


def _check_range(buf, off, length=None):  # SafeUtils.java:24-36
    if length is None:
        if off < 0 or off >= len(buf):
            raise IndexError(off)
        return
    _check_length(length)
    if length > 0:
        _check_range(buf, off)
        _check_range(buf, off + length - 1)


def _ro_ptr(buf):
    """(address, keepalive) of a readable bytes-like object"""
    if isinstance(buf, bytes):
        return C.cast(C.c_char_p(buf), C.c_void_p).value or 0, buf
    mv = memoryview(buf)
    if mv.readonly:
        b = bytes(mv)
        return C.cast(C.c_char_p(b), C.c_void_p).value or 0, b
    arr = (C.c_uint8 * max(len(mv), 1)).from_buffer(mv) if len(mv) else (C.c_uint8 * 1)()
    return C.addressof(arr), arr


def _rw_ptr(buf):
    mv = memoryview(buf)
    if mv.readonly:
        raise ReadOnlyBufferException("dest is read-only")
    arr = (C.c_uint8 * max(len(mv), 1)).from_buffer(mv) if len(mv) else (C.c_uint8 * 1)()
    return C.addressof(arr), arr


def maxCompressedLength(length):  # LZ4Utils.java:34-41
    if length < 0:
        raise ValueError("length must be >= 0, got %d" % length)
    if length >= 0x7E000000:
        raise ValueError("length must be < 0x7E000000")
    return length + length // 255 + 16


# ----------------------------------------------------------------------------------------------
# LZ4Compressor family
# ----------------------------------------------------------------------------------------------
class LZ4Compressor:
    """lz4/LZ4Compressor.java"""

    def maxCompressedLength(self, length):
        return maxCompressedLength(length)

    def _native(self, sp, src_len, dp, max_dest_len):
        raise NotImplementedError

    def compress(self, src, srcOff=None, srcLen=None, dest=None, destOff=None, maxDestLen=None):
        """compress(src) -> bytes | compress(src, srcOff, srcLen) -> bytes |
        compress(src, srcOff, srcLen, dest, destOff[, maxDestLen]) -> int  (LZ4Compressor.java:59-147)"""
        if dest is None:
            srcOff = 0 if srcOff is None else srcOff
            srcLen = len(src) - srcOff if srcLen is None else srcLen
            out = bytearray(self.maxCompressedLength(srcLen))
            n = self.compress(src, srcOff, srcLen, out, 0, len(out))
            return bytes(out[:n])
        destOff = 0 if destOff is None else destOff
        maxDestLen = len(dest) - destOff if maxDestLen is None else maxDestLen
        dp, dk = _rw_ptr(dest)                      # checkNotReadOnly(dest)
        _check_range(src, srcOff, srcLen)           # LZ4JNICompressor.java:36-37
        _check_range(dest, destOff, maxDestLen)
        sp, sk = _ro_ptr(src)
        result = self._native(sp + srcOff, srcLen, dp + destOff, maxDestLen)
        if result <= 0:
            raise LZ4Exception("maxDestLen is too small")
        return result


class LZ4HIPCompressor(LZ4Compressor):
    """twin of lz4/LZ4JNICompressor.java: fast compressor over lz4hip_compress_fast.  acceleration != 1: the bytes of liblz4's
    LZ4_compress_fast(..., acceleration) (lz4hip_compress_fast_accel; values below 1 act as 1, above 65537 as 65537)"""

    def __init__(self, acceleration=1):
        self.acceleration = int(acceleration)

    def _native(self, sp, src_len, dp, max_dest_len):
        if self.acceleration == 1:
            return _single(lib().lz4hip_compress_fast(sp, src_len, dp, max_dest_len))
        return _single(lib().lz4hip_compress_fast_accel(sp, src_len, dp, max_dest_len, self.acceleration))

    def compressDestSize(self, src, srcOff, srcLen, dest, destOff, targetDestSize):
        """liblz4's LZ4_compress_destSize: compresses as much of src[srcOff:srcOff+srcLen] as fits in exactly targetDestSize bytes
        at dest[destOff:] -> (written, consumed): the bytes written and the source bytes they cover (lz4hip_compress_dest_size).
        liblz4 has no accelerated destSize: an accelerated compressor raises NotImplementedError."""
        if self.acceleration > 1:
            raise NotImplementedError("compressDestSize: liblz4 has no accelerated destSize (acceleration %d)" % self.acceleration)
        dp, dk = _rw_ptr(dest)                      # the argument checks of compress()
        _check_range(src, srcOff, srcLen)
        _check_range(dest, destOff, targetDestSize)
        sp, sk = _ro_ptr(src)
        size = C.c_int32(srcLen)
        written = _single(lib().lz4hip_compress_dest_size(sp + srcOff, C.byref(size), dp + destOff, targetDestSize))
        return written, size.value

    def compressWithDict(self, dictionary, src, srcOff=None, srcLen=None, dest=None, destOff=None, maxDestLen=None):
        """liblz4's LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream (the dictionary not contiguous with src): the block
        src[srcOff:srcOff+srcLen] compressed alone against an LZ4Dictionary (lz4hip_compress_fast_dict); the forms of compress():
        compressWithDict(d, src[, srcOff, srcLen]) -> bytes | compressWithDict(d, src, srcOff, srcLen, dest, destOff[, maxDestLen]) -> int.
        LZ4SafeDecompressor.decompressWithDict reads it.  liblz4 has no accelerated form here: an accelerated compressor raises
        NotImplementedError."""
        if self.acceleration > 1:
            raise NotImplementedError("compressWithDict: acceleration %d is not supported" % self.acceleration)
        if dest is None:
            srcOff = 0 if srcOff is None else srcOff
            srcLen = len(src) - srcOff if srcLen is None else srcLen
            out = bytearray(self.maxCompressedLength(srcLen))
            n = self.compressWithDict(dictionary, src, srcOff, srcLen, out, 0, len(out))
            return bytes(out[:n])
        destOff = 0 if destOff is None else destOff
        maxDestLen = len(dest) - destOff if maxDestLen is None else maxDestLen
        dp, dk = _rw_ptr(dest)
        _check_range(src, srcOff, srcLen)
        _check_range(dest, destOff, maxDestLen)
        sp, sk = _ro_ptr(src)
        result = _single(lib().lz4hip_compress_fast_dict(sp + srcOff, srcLen, dp + destOff, maxDestLen, dictionary._handle()))
        if result <= 0:
            raise LZ4Exception("maxDestLen is too small")
        return result

    def __str__(self):
        return "LZ4HIPCompressor" if self.acceleration == 1 else "LZ4HIPCompressor(acceleration=%d)" % self.acceleration


class LZ4HCHIPCompressor(LZ4Compressor):
    """twin of lz4/LZ4HCJNICompressor.java:42-51 (level clamp: LZ4Factory.java:263-270)"""

    def __init__(self, compressionLevel=9):
        self.compressionLevel = compressionLevel

    def _native(self, sp, src_len, dp, max_dest_len):
        return _single(lib().lz4hip_compress_hc(sp, src_len, dp, max_dest_len, self.compressionLevel))

    def compress(self, src, srcOff=None, srcLen=None, dest=None, destOff=None, maxDestLen=None):
        try:
            return super().compress(src, srcOff, srcLen, dest, destOff, maxDestLen)
        except LZ4Exception:
            raise LZ4Exception()  # LZ4HCJNICompressor.java:47-49 throws without a message

    def compressDestSize(self, src, srcOff, srcLen, dest, destOff, targetDestSize):
        """liblz4's LZ4_compress_HC_destSize at this compressor's level: compresses as much of src[srcOff:srcOff+srcLen] as fits in
        exactly targetDestSize bytes at dest[destOff:] -> (written, consumed): the bytes written and the source bytes they cover
        (lz4hip_compress_hc_dest_size)."""
        dp, dk = _rw_ptr(dest)                      # the argument checks of compress()
        _check_range(src, srcOff, srcLen)
        _check_range(dest, destOff, targetDestSize)
        sp, sk = _ro_ptr(src)
        size = C.c_int32(srcLen)
        written = _single(lib().lz4hip_compress_hc_dest_size(sp + srcOff, C.byref(size), dp + destOff, targetDestSize, self.compressionLevel))
        return written, size.value

    def compressWithDict(self, dictionary, src, srcOff=None, srcLen=None, dest=None, destOff=None, maxDestLen=None):
        """liblz4's LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream at this compressor's level (the dictionary not
        contiguous with src): the block src[srcOff:srcOff+srcLen] compressed alone against an LZ4Dictionary (lz4hip_compress_hc_dict);
        the forms of compress(): compressWithDict(d, src[, srcOff, srcLen]) -> bytes | compressWithDict(d, src, srcOff, srcLen, dest,
        destOff[, maxDestLen]) -> int.  LZ4SafeDecompressor.decompressWithDict reads it."""
        if dest is None:
            srcOff = 0 if srcOff is None else srcOff
            srcLen = len(src) - srcOff if srcLen is None else srcLen
            out = bytearray(self.maxCompressedLength(srcLen))
            n = self.compressWithDict(dictionary, src, srcOff, srcLen, out, 0, len(out))
            return bytes(out[:n])
        destOff = 0 if destOff is None else destOff
        maxDestLen = len(dest) - destOff if maxDestLen is None else maxDestLen
        dp, dk = _rw_ptr(dest)
        _check_range(src, srcOff, srcLen)
        _check_range(dest, destOff, maxDestLen)
        sp, sk = _ro_ptr(src)
        result = _single(lib().lz4hip_compress_hc_dict(sp + srcOff, srcLen, dp + destOff, maxDestLen, self.compressionLevel, dictionary._handle()))
        if result <= 0:
            raise LZ4Exception()
        return result


# ----------------------------------------------------------------------------------------------
# decompressors
# ----------------------------------------------------------------------------------------------
class LZ4Dictionary:
    """A shared dictionary for LZ4_decompress_safe_usingDict, for LZ4_loadDict + LZ4_compress_fast_continue and for LZ4_loadDictHC +
    LZ4_compress_HC_continue (lz4hip_dict_create): the handle keeps the true length and the last 64 KB, resident on every initialised
    device (and, from its first compress on a device, the 32 KB table LZ4_loadDict leaves; from its first HC compress, the 128 KB head
    table and 2 bytes per kept byte that LZ4_loadDictHC leaves).  Immutable; any number of threads may compress and decode against it.  close() -- or leaving a `with`
    block -- frees it; no call that uses it may be in flight then."""

    def __init__(self, data):
        n = len(data)
        p, keep = _ro_ptr(data if n else b"\0")
        self._h = C.c_void_p(None)
        _chk(lib().lz4hip_dict_create(p, n, C.byref(self._h)))

    def _handle(self):
        if not self._h:
            raise AssertionError("Already closed")
        return self._h

    def __len__(self):
        return lib().lz4hip_dict_size(self._handle())

    def close(self):
        if self._h:
            lib().lz4hip_dict_free(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __repr__(self):
        return "LZ4Dictionary(%s)" % ("%d bytes" % len(self) if self._h else "closed")


class LZ4SafeDecompressor:
    """lz4/LZ4SafeDecompressor.java; JNI twin LZ4JNISafeDecompressor.java:34-43"""

    def decompress(self, src, srcOff=None, srcLen=None, dest=None, destOff=None, maxDestLen=None):
        """decompress(src, maxDestLen) -> bytes | decompress(src, srcOff, srcLen, maxDestLen) -> bytes |
        decompress(src, srcOff, srcLen, dest, destOff[, maxDestLen]) -> int"""
        if dest is None or isinstance(dest, int):
            if dest is None and srcLen is None:       # decompress(src, maxDestLen)
                max_len, srcOff, srcLen = srcOff, 0, len(src)
            else:                                      # decompress(src, srcOff, srcLen, maxDestLen)
                max_len = dest
            out = bytearray(max_len)
            n = self.decompress(src, srcOff, srcLen, out, 0, max_len)
            return bytes(out[:n])
        destOff = 0 if destOff is None else destOff
        maxDestLen = len(dest) - destOff if maxDestLen is None else maxDestLen
        dp, dk = _rw_ptr(dest)
        _check_range(src, srcOff, srcLen)
        _check_range(dest, destOff, maxDestLen)
        sp, sk = _ro_ptr(src)
        result = _single(lib().lz4hip_decompress_safe(sp + srcOff, srcLen, dp + destOff, maxDestLen))
        if result < 0:
            raise LZ4Exception("Error decoding offset %d of input buffer" % (srcOff - result))
        return result

    def decompressWithDict(self, dictionary, src, srcOff, srcLen, dest, destOff, maxDestLen=None):
        """liblz4's LZ4_decompress_safe_usingDict against an LZ4Dictionary (not contiguous with dest): decodes the block in
        src[srcOff:srcOff+srcLen], which was compressed against that dictionary, into dest[destOff:] and returns the decoded size
        (lz4hip_decompress_safe_dict)"""
        destOff = 0 if destOff is None else destOff
        maxDestLen = len(dest) - destOff if maxDestLen is None else maxDestLen
        dp, dk = _rw_ptr(dest)
        _check_range(src, srcOff, srcLen)
        _check_range(dest, destOff, maxDestLen)
        sp, sk = _ro_ptr(src)
        result = _single(lib().lz4hip_decompress_safe_dict(sp + srcOff, srcLen, dp + destOff, maxDestLen, dictionary._handle()))
        if result < 0:
            raise LZ4Exception("Error decoding offset %d of input buffer" % (srcOff - result))
        return result

    def decompressPartial(self, src, srcOff, srcLen, dest, destOff, targetLen, maxDestLen=None):
        """liblz4's LZ4_decompress_safe_partial: decodes the first min(targetLen, maxDestLen) bytes of the block in
        src[srcOff:srcOff+srcLen] (fewer where the stream ends first: a cut stream decodes to what its bytes hold) into dest[destOff:]
        and returns the count; nothing is written past destOff + min(targetLen, maxDestLen) (lz4hip_decompress_safe_partial)"""
        destOff = 0 if destOff is None else destOff
        maxDestLen = len(dest) - destOff if maxDestLen is None else maxDestLen
        dp, dk = _rw_ptr(dest)
        _check_range(src, srcOff, srcLen)
        _check_range(dest, destOff, maxDestLen)
        sp, sk = _ro_ptr(src)
        result = _single(lib().lz4hip_decompress_safe_partial(sp + srcOff, srcLen, dp + destOff, targetLen, maxDestLen))
        if result < 0:
            raise LZ4Exception("Error decoding offset %d of input buffer" % (srcOff - result))
        return result

    def decompressedLength(self, src, srcOff, srcLen, maxDestLen):
        """what decompress(src, srcOff, srcLen, dest, destOff, maxDestLen) would return -- the decoded size of the block in
        src[srcOff:srcOff+srcLen] for a destination of maxDestLen bytes -- without a destination: nothing is decoded into memory
        (lz4hip_decompressed_size).  A stream that decompress() rejects with that capacity raises the same LZ4Exception"""
        _check_range(src, srcOff, srcLen)
        _check_length(maxDestLen)
        sp, sk = _ro_ptr(src)
        result = _single(lib().lz4hip_decompressed_size(sp + srcOff, srcLen, maxDestLen))
        if result < 0:
            raise LZ4Exception("Error decoding offset %d of input buffer" % (srcOff - result))
        return result


class LZ4FastDecompressor:
    """lz4/LZ4FastDecompressor.java; JNI twin LZ4JNIFastDecompressor.java:35-44"""

    def decompress(self, src, srcOff=None, dest=None, destOff=None, destLen=None):
        """decompress(src, destLen) -> bytes | decompress(src, srcOff, destLen) -> bytes |
        decompress(src, srcOff, dest, destOff, destLen) -> int (bytes read from src)"""
        if dest is None or isinstance(dest, int):
            if dest is None:                           # decompress(src, destLen)
                dest_len, srcOff = srcOff, 0
            else:                                      # decompress(src, srcOff, destLen)
                dest_len = dest
            out = bytearray(dest_len)
            self.decompress(src, srcOff, out, 0, dest_len)
            return bytes(out)
        dp, dk = _rw_ptr(dest)
        _check_range(src, srcOff) if len(src) or srcOff else None
        _check_range(dest, destOff, destLen)
        sp, sk = _ro_ptr(src)
        result = _single(lib().lz4hip_decompress_fast(sp + srcOff, len(src) - srcOff, dp + destOff, destLen))
        if result < 0:
            raise LZ4Exception("Error decoding offset %d of input buffer" % (srcOff - result))
        return result


# ----------------------------------------------------------------------------------------------
# factory
# ----------------------------------------------------------------------------------------------
class LZ4Factory:
    """lz4/LZ4Factory.java -- only the new fourth accessor exists here (the other three families are
    the reference's own and are not rebuilt)."""

    _HIP = None

    def __init__(self, impl):
        if impl != "HIP":
            raise ValueError("only the HIP family lives in this package")
        self.impl = impl
        self._fast = LZ4HIPCompressor()
        self._hc = {}
        self._fast_dec = LZ4FastDecompressor()
        self._safe_dec = LZ4SafeDecompressor()
        # LZ4Factory.java:204-220: the constructor round-trips a 20-byte vector through all members
        original = b"abcd      abcdefghij"
        for compressor in (self._fast, self.highCompressor()):
            compressed = compressor.compress(original)
            if self._fast_dec.decompress(compressed, len(original)) != original:
                raise AssertionError("fast decompressor self-test failed")
            if self._safe_dec.decompress(compressed, len(original)) != original:
                raise AssertionError("safe decompressor self-test failed")

    @classmethod
    def hipInstance(cls):
        if cls._HIP is None:
            cls._HIP = cls("HIP")
        return cls._HIP

    def fastCompressor(self, acceleration=1):
        """acceleration 1 (the default): the factory's compressor; any other value: a compressor bound to it (LZ4_compress_fast)"""
        if acceleration == 1:
            return self._fast
        return LZ4HIPCompressor(acceleration)

    def highCompressor(self, compressionLevel=9):
        if compressionLevel > 17:
            compressionLevel = 17
        elif compressionLevel < 1:
            compressionLevel = 9
        if compressionLevel not in self._hc:
            self._hc[compressionLevel] = LZ4HCHIPCompressor(compressionLevel)
        return self._hc[compressionLevel]

    def fastDecompressor(self):
        return self._fast_dec

    def safeDecompressor(self):
        return self._safe_dec

    def __str__(self):
        return "LZ4Factory:HIP"


# ----------------------------------------------------------------------------------------------
# xxhash
# ----------------------------------------------------------------------------------------------
class XXHash32:
    """xxhash/XXHash32.java:38; JNI twin XXHash32JNI.java:29-33"""

    def hash(self, buf, off=0, length=None, seed=0):
        length = len(buf) - off if length is None else length
        _check_range(buf, off, length)
        p, k = _ro_ptr(buf)
        out = C.c_uint32(0)
        _chk(lib().lz4hip_xxh32(p + off, length, seed & 0xFFFFFFFF, C.byref(out)))
        return out.value


class XXHash64:
    """xxhash/XXHash64.java:38; JNI twin XXHash64JNI.java:29-33"""

    def hash(self, buf, off=0, length=None, seed=0):
        length = len(buf) - off if length is None else length
        _check_range(buf, off, length)
        p, k = _ro_ptr(buf)
        out = C.c_uint64(0)
        _chk(lib().lz4hip_xxh64(p + off, length, seed & 0xFFFFFFFFFFFFFFFF, C.byref(out)))
        return out.value


class _Checksum:
    """java.util.zip.Checksum view of a streaming hash (StreamingXXHash32.java:96-126, StreamingXXHash64.java:96-126)"""

    def __init__(self, h, mask):
        self._h, self._mask = h, mask

    def getValue(self):
        return self._h.getValue() & self._mask

    def reset(self):
        self._h.reset()

    def update(self, b, off=None, length=None):
        if isinstance(b, int):
            self._h.update(bytes([b & 0xFF]), 0, 1)
        else:
            self._h.update(b, 0 if off is None else off, (len(b) if off is None else len(b) - off) if length is None else length)


class _StreamingXXHash:
    """Common part of the streaming twins: the state is a record in device memory behind a lz4hip_xxh_stream handle;
    update() continues it with one launch; getValue() may be called any number of times between updates."""

    _IS64 = False

    def __init__(self, seed):
        self.seed = seed
        self._state = C.c_void_p(None)
        if self._IS64:
            _chk(lib().lz4hip_xxh64_stream_create(seed & 0xFFFFFFFFFFFFFFFF, C.byref(self._state)))
        else:
            _chk(lib().lz4hip_xxh32_stream_create(seed & 0xFFFFFFFF, C.byref(self._state)))

    def _check_state(self):  # StreamingXXHash32JNI.java:47-51
        if not self._state:
            raise AssertionError("Already finalized")

    def reset(self):
        self._check_state()
        _chk(lib().lz4hip_xxh_stream_reset(self._state, self.seed & 0xFFFFFFFFFFFFFFFF))

    def update(self, buf, off=0, length=None):
        self._check_state()
        length = len(buf) - off if length is None else length
        _check_range(buf, off, length)
        p, k = _ro_ptr(buf)
        _chk(lib().lz4hip_xxh_stream_update(self._state, p + off, length))

    def update_device(self, dptr, length, stream=None):
        """Not in the reference: absorbs `length` bytes at DEVICE address `dptr` where they lie (asynchronous on `stream`)."""
        self._check_state()
        if length < 0:
            raise IndexError("length must be >= 0")
        _chk(lib().lz4hip_xxh_stream_update_dev(self._state, dptr, length, stream))

    def close(self):
        if self._state:
            lib().lz4hip_xxh_stream_free(self._state)
            self._state = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __repr__(self):
        return "%s(seed=%d)" % (type(self).__name__, self.seed)


class StreamingXXHash32(_StreamingXXHash):
    """xxhash/StreamingXXHash32.java:38-129; JNI twin StreamingXXHash32JNI.java:28-104 (XXH32_init/_update/_digest/_free)"""

    def getValue(self):
        self._check_state()
        out = C.c_uint32(0)
        _chk(lib().lz4hip_xxh32_stream_digest(self._state, C.byref(out)))
        return out.value

    def asChecksum(self):
        return _Checksum(self, 0xFFFFFFF)  # 28 bits: StreamingXXHash32.java:101-107


class StreamingXXHash64(_StreamingXXHash):
    """xxhash/StreamingXXHash64.java:38-129; JNI twin StreamingXXHash64JNI.java:28-104"""

    _IS64 = True

    def getValue(self):
        self._check_state()
        out = C.c_uint64(0)
        _chk(lib().lz4hip_xxh64_stream_digest(self._state, C.byref(out)))
        return out.value

    def asChecksum(self):
        return _Checksum(self, 0xFFFFFFFFFFFFFFFF)


class XXHashFactory:
    """xxhash/XXHashFactory.java: hash32() / hash64() one-shot hashes, newStreamingHash32/64(seed) streaming states"""

    _HIP = None

    @classmethod
    def hipInstance(cls):
        if cls._HIP is None:
            cls._HIP = cls()
        return cls._HIP

    def hash32(self):
        return XXHash32()

    def hash64(self):
        return XXHash64()

    def newStreamingHash32(self, seed):  # XXHashFactory.java:230-232
        return StreamingXXHash32(seed)

    def newStreamingHash64(self, seed):  # XXHashFactory.java:240-242
        return StreamingXXHash64(seed)


# ----------------------------------------------------------------------------------------------
# batch helper (host memory)
# ----------------------------------------------------------------------------------------------
def _arr(ctype, values):
    """ctypes array of the per-block offsets / lengths; a numpy array of the matching width is used in place (no copy)"""
    n = len(values)
    if hasattr(values, "ctypes") and hasattr(values, "dtype") and values.dtype.itemsize == C.sizeof(ctype) and \
            values.dtype.kind in "iu" and values.flags["C_CONTIGUOUS"] and n:
        return (ctype * n).from_address(values.ctypes.data)   # (the caller's array outlives the call)
    return (ctype * max(n, 1))(*values)


class LZ4HIPBatch:
    """Many independent blocks per launch -- the entry point the reference lacks.
    `src`/`dst` are single host buffers; block i lives at src[srcOff[i]:+srcLen[i]] and owns the
    slot dst[dstOff[i]:+dstCap[i]]."""

    @staticmethod
    def _check_ranges(buf, off, length):
        """SafeUtils.checkRange for every block: 0 <= off and off + len <= len(buf) (for decompressFast `length` is the readable
        capacity of the slot -- it bounds what the engine may read, so it must lie inside the buffer like any other range)"""
        n = len(off)
        if hasattr(off, "dtype") or hasattr(length, "dtype"):
            import numpy as np
            o, l = np.asarray(off, dtype=np.int64), np.asarray(length, dtype=np.int64)
            if n and ((l < 0).any() or (o < 0).any() or ((o + l) > len(buf)).any()):
                raise IndexError("block range outside its buffer")
        else:
            for i in range(n):
                _check_range(buf, off[i], length[i])

    @classmethod
    def _call(cls, fn, src, srcOff, srcLen, dst, dstOff, dstCap, *extra):
        n = len(srcOff)
        if not (len(srcLen) == len(dstOff) == len(dstCap) == n):
            raise ValueError("per-block arrays differ in length")
        cls._check_ranges(src, srcOff, srcLen)
        cls._check_ranges(dst, dstOff, dstCap)
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        _chk(getattr(lib(), fn)(sp, _arr(C.c_uint64, srcOff), _arr(C.c_int32, srcLen), dp, _arr(C.c_uint64, dstOff),
                                _arr(C.c_int32, dstCap), out, n, *extra))
        if hasattr(srcOff, "dtype"):
            import numpy as np
            return np.frombuffer(out, dtype=np.int32, count=n).copy()
        return list(out[:n])

    @classmethod
    def compress(cls, src, srcOff, srcLen, dst, dstOff, dstCap, acceleration=1):
        """acceleration != 1: LZ4_compress_fast(..., acceleration) per block (lz4hip_compress_fast_accel_batch)"""
        if acceleration == 1:
            return cls._call("lz4hip_compress_fast_batch", src, srcOff, srcLen, dst, dstOff, dstCap)
        return cls._call("lz4hip_compress_fast_accel_batch", src, srcOff, srcLen, dst, dstOff, dstCap, int(acceleration))

    @classmethod
    def compressDestSize(cls, src, srcOff, srcLen, dst, dstOff, targetSize):
        """LZ4_compress_destSize per block: as much of block i as fits in exactly targetSize[i] bytes at dst[dstOff[i]:]
        -> (outLen, srcConsumed) (lz4hip_compress_dest_size_batch; lists, or int32 arrays for numpy inputs)"""
        n = len(srcOff)
        if not (len(srcLen) == len(dstOff) == len(targetSize) == n):
            raise ValueError("per-block arrays differ in length")
        cls._check_ranges(src, srcOff, srcLen)
        cls._check_ranges(dst, dstOff, targetSize)
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        consumed = (C.c_int32 * max(n, 1))()
        _chk(lib().lz4hip_compress_dest_size_batch(sp, _arr(C.c_uint64, srcOff), _arr(C.c_int32, srcLen), dp, _arr(C.c_uint64, dstOff),
                                                   _arr(C.c_int32, targetSize), out, consumed, n))
        if hasattr(srcOff, "dtype"):
            import numpy as np
            return (np.frombuffer(out, dtype=np.int32, count=n).copy(), np.frombuffer(consumed, dtype=np.int32, count=n).copy())
        return list(out[:n]), list(consumed[:n])

    @classmethod
    def compressHC(cls, src, srcOff, srcLen, dst, dstOff, dstCap, level=9):
        n = len(srcOff)
        if not (len(srcLen) == len(dstOff) == len(dstCap) == n):
            raise ValueError("per-block arrays differ in length")
        cls._check_ranges(src, srcOff, srcLen)
        cls._check_ranges(dst, dstOff, dstCap)
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        _chk(lib().lz4hip_compress_hc_batch(sp, _arr(C.c_uint64, srcOff), _arr(C.c_int32, srcLen), dp, _arr(C.c_uint64, dstOff),
                                            _arr(C.c_int32, dstCap), out, n, level))
        return list(out[:n])

    @classmethod
    def compressHCDestSize(cls, src, srcOff, srcLen, dst, dstOff, targetSize, level=9):
        """LZ4_compress_HC_destSize per block at HC level `level`: as much of block i as fits in exactly targetSize[i] bytes at
        dst[dstOff[i]:] -> (outLen, srcConsumed) (lz4hip_compress_hc_dest_size_batch; lists, or int32 arrays for numpy inputs)"""
        n = len(srcOff)
        if not (len(srcLen) == len(dstOff) == len(targetSize) == n):
            raise ValueError("per-block arrays differ in length")
        cls._check_ranges(src, srcOff, srcLen)
        cls._check_ranges(dst, dstOff, targetSize)
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        consumed = (C.c_int32 * max(n, 1))()
        _chk(lib().lz4hip_compress_hc_dest_size_batch(sp, _arr(C.c_uint64, srcOff), _arr(C.c_int32, srcLen), dp, _arr(C.c_uint64, dstOff),
                                                      _arr(C.c_int32, targetSize), out, consumed, n, int(level)))
        if hasattr(srcOff, "dtype"):
            import numpy as np
            return (np.frombuffer(out, dtype=np.int32, count=n).copy(), np.frombuffer(consumed, dtype=np.int32, count=n).copy())
        return list(out[:n]), list(consumed[:n])

    FRAME_BLOCKS, LZ4BLOCK_BLOCKS = 0, 1

    @staticmethod
    def containerBlocks(kind, data, blockSize, blockChecksum=False, level=0):
        """the data blocks of an LZ4 Frame (kind FRAME_BLOCKS) or of lz4-java's LZ4Block container (LZ4BLOCK_BLOCKS) for `data` cut
        into blockSize pieces, assembled on the device (compress, raw fallback, headers, compaction, checksums): the bytes the
        reference's LZ4FrameOutputStream.writeBlock / LZ4BlockOutputStream.flushBufferedData emit for the same blocks"""
        n = (len(data) + blockSize - 1) // blockSize
        cap = len(data) + n * (8 if kind == 0 else 21)
        dst = bytearray(max(cap, 1))
        sp, sk = _ro_ptr(data)
        dp, dk = _rw_ptr(dst)
        out = C.c_uint64(0)
        _chk(lib().lz4hip_container_blocks(kind, 1 if blockChecksum else 0, level, sp, len(data), blockSize, dp, cap, C.byref(out)))
        return bytes(dst[:out.value])

    @staticmethod
    def containerBlocksManyBound(kind, lengths, blockSizes, blockChecksums=False, gapHead=0, gapTail=0):
        """lz4hip_container_blocks_many_bound (no device): per item (blocks, worst-case bytes with its gaps)"""
        import numpy as np
        n = len(lengths)
        per = lambda v, t: np.asarray(list(v) if hasattr(v, "__len__") else [v] * n, dtype=t)
        ln, bs, gh, gt = per(lengths, np.uint64), per(blockSizes, np.uint32), per(gapHead, np.uint32), per(gapTail, np.uint32)
        fl = np.asarray([1 if c else 0 for c in (blockChecksums if hasattr(blockChecksums, "__len__") else [blockChecksums] * n)], dtype=np.uint8)
        if not (len(ln) == len(bs) == len(gh) == len(gt) == len(fl) == n):
            raise ValueError("per-item lists differ in length")
        a = lambda v, t: v.ctypes.data_as(C.POINTER(t))
        nbs, need = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint64)
        _chk(lib().lz4hip_container_blocks_many_bound(kind, a(ln, C.c_uint64), a(bs, C.c_uint32), a(fl, C.c_uint8), a(gh, C.c_uint32), a(gt, C.c_uint32), n,
                                                      a(nbs, C.c_uint32), a(need, C.c_uint64)))
        return [(int(nbs[c]), int(need[c])) for c in range(n)]

    @staticmethod
    def containerBlocksMany(kind, items, blockSizes, blockChecksums=False, level=0, gapHead=0, gapTail=0, contentHash=False):
        """containerBlocks for MANY payloads of one kind in one call (lz4hip_container_blocks_many): `items` is a list of payloads;
        blockSizes, blockChecksums, gapHead, gapTail and contentHash are lists of the same length (or one value for all).  ->
        (dst, off, hashes): item c's bytes are dst[off[c]:off[c + 1]] (a writable numpy uint8 array): gapHead[c] zero bytes, the bytes
        containerBlocks(kind, items[c], blockSizes[c], blockChecksums[c], level) returns, gapTail[c] zero bytes; hashes[c] is the XXH32
        (seed 0) of items[c] where contentHash[c] is set, else 0.  A group of items costs one launch sequence, whatever their number"""
        import numpy as np
        n = len(items)
        per = lambda v: list(v) if hasattr(v, "__len__") else [v] * n
        bsl, ckl, ghl, gtl, chl = per(blockSizes), per(blockChecksums), per(gapHead), per(gapTail), per(contentHash)
        if not (len(bsl) == len(ckl) == len(ghl) == len(gtl) == len(chl) == n):
            raise ValueError("per-item lists differ in length")
        doff = np.zeros(n + 1, dtype=np.uint64)
        if n == 0:
            return np.zeros(0, dtype=np.uint8), doff, np.zeros(0, dtype=np.uint32)
        lens = np.fromiter((len(b) for b in items), dtype=np.uint64, count=n)
        offs = np.zeros(n, dtype=np.uint64)
        np.cumsum(lens[:-1], out=offs[1:])
        blob = b"".join(bytes(b) if not isinstance(b, (bytes, bytearray)) else b for b in items)
        sp, sk = _ro_ptr(blob if blob else b"\0")
        bs, gh, gt = np.asarray(bsl, dtype=np.uint32), np.asarray(ghl, dtype=np.uint32), np.asarray(gtl, dtype=np.uint32)
        fl = np.asarray([(1 if c else 0) | (2 if h else 0) for c, h in zip(ckl, chl)], dtype=np.uint8)
        a = lambda v, t: v.ctypes.data_as(C.POINTER(t))
        nbs, need = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        _chk(lib().lz4hip_container_blocks_many_bound(kind, a(lens, C.c_uint64), a(bs, C.c_uint32), a(fl, C.c_uint8), a(gh, C.c_uint32), a(gt, C.c_uint32), n,
                                                      a(nbs, C.c_uint32), a(need, C.c_uint64)))
        cap = int(need.sum())
        dst = np.empty(max(cap, 1), dtype=np.uint8)
        hashes = np.zeros(n, dtype=np.uint32)
        _chk(lib().lz4hip_container_blocks_many(kind, level, sp, a(offs, C.c_uint64), a(lens, C.c_uint64), a(bs, C.c_uint32), a(fl, C.c_uint8),
                                                a(gh, C.c_uint32), a(gt, C.c_uint32), n, a(dst, C.c_uint8), cap, a(doff, C.c_uint64), a(hashes, C.c_uint32)))
        return dst, doff, hashes

    # stop reasons of containerDecode (include/lz4hip.h)
    CR_END, CR_MORE, CR_TRUNCATED, CR_BLOCK_TOO_BIG, CR_BLOCK_CHECKSUM, CR_DECODE, CR_CORRUPT, CR_SLOTS = range(8)

    @staticmethod
    def containerDecode(kind, body, maxBlock, nMax, blockChecksum=False):
        """the READ path of the container formats on the device: the data blocks of an LZ4 Frame body / of an LZ4Block stream in `body`
        are walked, verified and decoded there (LZ4FrameInputStream.readBlock / LZ4BlockInputStream.refill for a run of blocks)
        -> (decoded bytes of the delivered blocks, [their sizes], bytes of body consumed, stop reason, liblz4 code of a failed decode)"""
        sp, sk = _ro_ptr(body)
        nb, need = C.c_uint32(0), C.c_uint64(0)   # the destination by what the body holds, not by nMax x maxBlock (round-4 advisor)
        _chk(lib().lz4hip_container_decode_bound(kind, 1 if blockChecksum else 0, sp, len(body), maxBlock, nMax, C.byref(nb), C.byref(need)))
        dst = bytearray(max(need.value, 1))
        sizes = (C.c_int32 * nMax)()
        info = (C.c_uint64 * 5)()
        dp, dk = _rw_ptr(dst)
        _chk(lib().lz4hip_container_decode(kind, 1 if blockChecksum else 0, sp, len(body), maxBlock, nMax, dp, len(dst), sizes, info))
        n_ok, consumed, why, total, code = (int(info[i]) for i in range(5))
        if code >= 1 << 63:
            code -= 1 << 64
        return bytes(dst[:total]), [int(sizes[i]) for i in range(n_ok)], consumed, why, code

    @staticmethod
    def containerDecodeMany(kind, bodies, maxBlock, nMax, blockChecksum=False):
        """containerDecode for MANY containers of one kind in one call (lz4hip_container_decode_many): `bodies` is a list of bodies,
        maxBlock and blockChecksum lists of the same length (or one value for all) -> per item the tuple containerDecode returns.
        A group of items costs one launch sequence, whatever their number; an item that stops changes nothing about another"""
        import numpy as np
        n = len(bodies)
        mb = list(maxBlock) if hasattr(maxBlock, "__len__") else [maxBlock] * n
        ck = list(blockChecksum) if hasattr(blockChecksum, "__len__") else [blockChecksum] * n
        if not (len(mb) == len(ck) == n):
            raise ValueError("per-item lists differ in length")
        if n == 0:
            return []
        lens = np.fromiter((len(b) for b in bodies), dtype=np.uint64, count=n)
        offs = np.zeros(n, dtype=np.uint64)
        np.cumsum(lens[:-1], out=offs[1:])
        blob = b"".join(bytes(b) if not isinstance(b, (bytes, bytearray)) else b for b in bodies)
        sp, sk = _ro_ptr(blob if blob else b"\0")
        mbs, fl = np.asarray(mb, dtype=np.uint32), np.asarray([1 if c else 0 for c in ck], dtype=np.uint8)
        a = lambda v, t: v.ctypes.data_as(C.POINTER(t))
        head = (kind, sp, a(offs, C.c_uint64), a(lens, C.c_uint64), a(mbs, C.c_uint32), a(fl, C.c_uint8), n, nMax)
        nbs, need = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        _chk(lib().lz4hip_container_decode_many_bound(*head, a(nbs, C.c_uint32), a(need, C.c_uint64)))
        cap, scap = int(need.sum()), int(nbs.sum())
        dst = np.empty(max(cap, 1), dtype=np.uint8)
        sizes, info = np.zeros(max(scap, 1), dtype=np.int32), np.zeros(5 * n, dtype=np.uint64)
        doff, first = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint32)
        _chk(lib().lz4hip_container_decode_many(*head, a(dst, C.c_uint8), cap, a(doff, C.c_uint64), a(first, C.c_uint32), a(sizes, C.c_int32), scap,
                                                a(info, C.c_uint64)))
        out = []
        for c in range(n):
            n_ok, consumed, why, total, code = (int(v) for v in info[5 * c:5 * c + 5])
            if code >= 1 << 63:
                code -= 1 << 64
            assert int(first[c + 1] - first[c]) == n_ok and int(doff[c + 1] - doff[c]) == total
            out.append((dst[int(doff[c]):int(doff[c + 1])].tobytes(), [int(v) for v in sizes[int(first[c]):int(first[c + 1])]], consumed, why, code))
        return out

    @classmethod
    def decompressSafe(cls, src, srcOff, srcLen, dst, dstOff, dstCap):
        return cls._call("lz4hip_decompress_safe_batch", src, srcOff, srcLen, dst, dstOff, dstCap)

    @classmethod
    def decompressFast(cls, src, srcOff, srcCap, dst, dstOff, dstLen):
        return cls._call("lz4hip_decompress_fast_batch", src, srcOff, srcCap, dst, dstOff, dstLen)

    @classmethod
    def compressDict(cls, src, srcOff, srcLen, dst, dstOff, dstCap, dictionary):
        """LZ4_loadDict + LZ4_compress_fast_continue per block, a fresh stream each, against one LZ4Dictionary -> compressed sizes,
        0 where dstCap[i] is too small (lz4hip_compress_fast_dict_batch)"""
        return cls._call("lz4hip_compress_fast_dict_batch", src, srcOff, srcLen, dst, dstOff, dstCap, dictionary._handle())

    @classmethod
    def compressHCDict(cls, src, srcOff, srcLen, dst, dstOff, dstCap, dictionary, level=9):
        """LZ4_loadDictHC + LZ4_compress_HC_continue per block at HC level `level`, a fresh stream each, against one LZ4Dictionary ->
        compressed sizes, 0 where liblz4 returns 0 (lz4hip_compress_hc_dict_batch)"""
        return cls._call("lz4hip_compress_hc_dict_batch", src, srcOff, srcLen, dst, dstOff, dstCap, int(level), dictionary._handle())

    @classmethod
    def decompressSafeDict(cls, src, srcOff, srcLen, dst, dstOff, dstCap, dictionary):
        """LZ4_decompress_safe_usingDict per block against one LZ4Dictionary -> liblz4's return values
        (lz4hip_decompress_safe_dict_batch)"""
        return cls._call("lz4hip_decompress_safe_dict_batch", src, srcOff, srcLen, dst, dstOff, dstCap, dictionary._handle())

    CHAIN_STOPPED = _INT32_MIN + 6   # LZ4HIP_CHAIN_STOPPED: a block behind its chain's first failed block

    @classmethod
    def decompressSafeChain(cls, src, srcOff, srcLen, dstCap, chainFirst, dst, chainDstOff, chainDstCap, chainPrefixLen=None, stored=None):
        """LZ4_decompress_safe_continue over chains of linked blocks (lz4hip_decompress_safe_chain_batch): chain c is the blocks
        chainFirst[c] .. chainFirst[c + 1] - 1, decoded back to back into dst[chainDstOff[c]:+chainDstCap[c]] behind
        chainPrefixLen[c] bytes of history that lie in front of it in dst (None: no history); dstCap[i] is the capacity liblz4 would be
        given for block i, stored[i] (None: no block is) marks a raw block that is copied -> (outLen, chainOutLen): liblz4's return
        value per block (CHAIN_STOPPED behind a chain's first negative one) and the bytes each chain decoded (lists, or int32 / uint64
        arrays for numpy inputs)"""
        n, nc = len(srcOff), len(chainDstOff)
        if not (len(srcLen) == len(dstCap) == n) or (stored is not None and len(stored) != n):
            raise ValueError("per-block arrays differ in length")
        if len(chainFirst) != nc + 1 or len(chainDstCap) != nc or (chainPrefixLen is not None and len(chainPrefixLen) != nc):
            raise ValueError("per-chain arrays differ in length")
        cls._check_ranges(src, srcOff, srcLen)
        for c in dstCap:
            _check_length(c)
        cls._check_ranges(dst, chainDstOff, chainDstCap)
        prev = 0
        for c in range(nc + 1):
            if chainFirst[c] < prev or (c == 0 and chainFirst[0] != 0):
                raise ValueError("chainFirst must ascend from 0 to the number of blocks")
            prev = chainFirst[c]
        if prev != n:
            raise ValueError("chainFirst must ascend from 0 to the number of blocks")
        if chainPrefixLen is not None:
            for c in range(nc):
                _check_length(chainPrefixLen[c])
                if chainPrefixLen[c] > chainDstOff[c]:
                    raise IndexError("history reaches in front of the buffer")
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        cout = (C.c_uint64 * max(nc, 1))()
        st = _arr(C.c_uint8, [1 if x else 0 for x in stored]) if stored is not None else None
        pre = _arr(C.c_int32, chainPrefixLen) if chainPrefixLen is not None else None
        _chk(lib().lz4hip_decompress_safe_chain_batch(sp, _arr(C.c_uint64, srcOff), _arr(C.c_int32, srcLen), st, _arr(C.c_int32, dstCap),
                                                      _arr(C.c_uint32, chainFirst), dp, _arr(C.c_uint64, chainDstOff), _arr(C.c_uint64, chainDstCap),
                                                      pre, out, cout, n, nc))
        if hasattr(srcOff, "dtype"):
            import numpy as np
            return np.frombuffer(out, dtype=np.int32, count=n).copy(), np.frombuffer(cout, dtype=np.uint64, count=nc).copy()
        return list(out[:n]), list(cout[:nc])

    @classmethod
    def decompressSafeStream(cls, state, src, srcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainWinOff, chainWinLen, inOrder=False):
        """LZ4_decompress_safe_continue on streams whose blocks land anywhere -- rings, alternating buffers, save areas, dictionaries
        elsewhere (lz4hip_decompress_safe_stream_batch): stream c is the blocks chainFirst[c] .. chainFirst[c + 1] - 1 of this call,
        block i is decoded to dst[dstOff[i]:+dstCap[i]], inside the stream's window dst[chainWinOff[c]:+chainWinLen[c]].  state[c] is
        the stream's (prefixEnd, prefixLen, extEnd, extLen) as offsets into dst -- (0, 0, 0, 0) is a fresh stream,
        LZ4_setStreamDecode(dst + p, n) is (p + n, n, 0, 0) -> (outLen, newState): liblz4's return value per block (CHAIN_STOPPED
        behind a stream's first negative one; a list, or an int32 array for numpy inputs) and the list of the streams' states behind
        the call, to be handed to the next one.  DecodeStreams keeps the states for its caller.  inOrder=True is the twin
        lz4hip_decompress_safe_stream_inorder_batch: the same call for streams whose slots overlap the history they can reach -- the ring
        of decoderRingBufferSize(maxBlock) bytes, small rings kept in step with the writer's -- where the bytes are the plain
        byte-forward definition's (include/lz4hip.h says when those are liblz4's); the two may alternate on one stream"""
        n, nc = len(srcOff), len(state)
        if not (len(srcLen) == len(dstOff) == len(dstCap) == n):
            raise ValueError("per-block arrays differ in length")
        if len(chainFirst) != nc + 1 or len(chainWinOff) != nc or len(chainWinLen) != nc:
            raise ValueError("per-stream arrays differ in length")
        cls._check_ranges(src, srcOff, srcLen)
        cls._check_ranges(dst, dstOff, dstCap)
        cls._check_ranges(dst, chainWinOff, chainWinLen)
        prev = 0
        for c in range(nc + 1):
            if chainFirst[c] < prev or (c == 0 and chainFirst[0] != 0):
                raise ValueError("chainFirst must ascend from 0 to the number of blocks")
            prev = chainFirst[c]
        if prev != n:
            raise ValueError("chainFirst must ascend from 0 to the number of blocks")
        flat = (C.c_uint64 * max(4 * nc, 1))()
        for c in range(nc):
            pe, pl, ee, el = (int(v) for v in state[c])
            if min(pe, pl, ee, el) < 0 or pl > pe or el > ee or (pl and pe > len(dst)) or (el and ee > len(dst)):
                raise IndexError("history outside the buffer")
            flat[4 * c:4 * c + 4] = (pe, pl, ee, el)
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        call = lib().lz4hip_decompress_safe_stream_inorder_batch if inOrder else lib().lz4hip_decompress_safe_stream_batch
        _chk(call(flat, sp, _arr(C.c_uint64, srcOff), _arr(C.c_int32, srcLen), _arr(C.c_uint32, chainFirst), dp,
                  _arr(C.c_uint64, dstOff), _arr(C.c_int32, dstCap), _arr(C.c_uint64, chainWinOff),
                  _arr(C.c_uint64, chainWinLen), out, n, nc))
        new = [tuple(flat[4 * c:4 * c + 4]) for c in range(nc)]
        if hasattr(srcOff, "dtype"):
            import numpy as np
            return np.frombuffer(out, dtype=np.int32, count=n).copy(), new
        return list(out[:n]), new

    @classmethod
    def _check_chains(cls, src, chainSrcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainPrefixLen):
        """the argument checks of the chain compressors -> (blocks, chains)"""
        n, nc = len(srcLen), len(chainSrcOff)
        if not (len(dstOff) == len(dstCap) == n):
            raise ValueError("per-block arrays differ in length")
        if len(chainFirst) != nc + 1 or (chainPrefixLen is not None and len(chainPrefixLen) != nc):
            raise ValueError("per-chain arrays differ in length")
        prev = 0
        for c in range(nc + 1):
            if chainFirst[c] < prev or (c == 0 and chainFirst[0] != 0):
                raise ValueError("chainFirst must ascend from 0 to the number of blocks")
            prev = chainFirst[c]
        if prev != n:
            raise ValueError("chainFirst must ascend from 0 to the number of blocks")
        for c in range(nc):
            total = 0
            for i in range(chainFirst[c], chainFirst[c + 1]):
                _check_length(srcLen[i])
                total += srcLen[i]
            _check_range(src, chainSrcOff[c], total)
            if chainSrcOff[c] < 0 or chainSrcOff[c] > len(src):
                raise IndexError(chainSrcOff[c])
            if chainPrefixLen is not None:
                _check_length(chainPrefixLen[c])
                if chainPrefixLen[c] > chainSrcOff[c]:
                    raise IndexError("history reaches in front of the buffer")
        cls._check_ranges(dst, dstOff, dstCap)
        return n, nc

    @classmethod
    def compressHCChain(cls, src, chainSrcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainPrefixLen=None, level=9):
        """LZ4_compress_HC_continue over chains of linked blocks, prefix mode (lz4hip_compress_hc_chain_batch): the arrays of
        compressFastChain and an HC level (< 1 -> 9, > 12 -> 12) -> outLen: liblz4's return value per block (a list, or an int32 array
        for numpy inputs).  A block whose result is 0 -- it did not fit -- does NOT end its chain: its source is history for the blocks
        behind it, and there is no CHAIN_STOPPED here.  Not serial: every block of every chain is parsed at once"""
        n, nc = cls._check_chains(src, chainSrcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainPrefixLen)
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        pre = _arr(C.c_int32, chainPrefixLen) if chainPrefixLen is not None else None
        _chk(lib().lz4hip_compress_hc_chain_batch(sp, _arr(C.c_uint64, chainSrcOff), pre, _arr(C.c_int32, srcLen), _arr(C.c_uint32, chainFirst), dp,
                                                  _arr(C.c_uint64, dstOff), _arr(C.c_int32, dstCap), out, n, nc, int(level)))
        if hasattr(srcLen, "dtype"):
            import numpy as np
            return np.frombuffer(out, dtype=np.int32, count=n).copy()
        return list(out[:n])

    @classmethod
    def compressHCStream(cls, state, src, srcOff, srcLen, chainFirst, dst, dstOff, dstCap, level=9):
        """LZ4_compress_HC_continue on streams whose sources land anywhere -- a ring that wraps, alternating buffers, a save area, a
        dictionary elsewhere (lz4hip_compress_hc_stream_batch): stream c is the blocks chainFirst[c] .. chainFirst[c + 1] - 1 of this
        call, block i is src[srcOff[i]:+srcLen[i]] and owns the slot dst[dstOff[i]:+dstCap[i]].  state[c] is the stream's (prefixEnd,
        prefixLen, extEnd, extLen, index) as offsets into src -- five zeros are a fresh stream -> (outLen, newState): liblz4's return
        value per block (0: it did not fit, which does not end the stream; a list, or an int32 array for numpy inputs) and the states
        behind the call, to be handed to the next one.  A call is a snapshot of src.  CompressStreamsHC keeps the states for its
        caller"""
        n, nc = len(srcOff), len(state)
        if not (len(srcLen) == len(dstOff) == len(dstCap) == n):
            raise ValueError("per-block arrays differ in length")
        if len(chainFirst) != nc + 1:
            raise ValueError("per-stream arrays differ in length")
        for i in range(n):
            if 0 <= srcLen[i] <= 0x7E000000:   # (any other length gives 0 and reads nothing: the engine's rule)
                _check_range(src, srcOff[i], srcLen[i])
            elif srcOff[i] < 0 or srcOff[i] > len(src):
                raise IndexError(srcOff[i])
        cls._check_ranges(dst, dstOff, [max(int(c), 0) for c in dstCap])
        flat = (C.c_uint64 * max(5 * nc, 1))()
        for c in range(nc):
            pe, pl, ee, el, ix = (int(v) for v in state[c])
            if min(pe, pl, ee, el, ix) < 0 or (pl and pe > len(src)) or (el and ee > len(src)):
                raise IndexError("history outside the buffer")
            flat[5 * c:5 * c + 5] = (pe, pl, ee, el, ix)
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        _chk(lib().lz4hip_compress_hc_stream_batch(flat, sp, _arr(C.c_uint64, srcOff), _arr(C.c_int32, srcLen), _arr(C.c_uint32, chainFirst), dp,
                                                   _arr(C.c_uint64, dstOff), _arr(C.c_int32, dstCap), out, n, nc, int(level)))
        new = [tuple(flat[5 * c:5 * c + 5]) for c in range(nc)]
        if hasattr(srcLen, "dtype"):
            import numpy as np
            return np.frombuffer(out, dtype=np.int32, count=n).copy(), new
        return list(out[:n]), new

    @classmethod
    def compressFastChain(cls, src, chainSrcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainPrefixLen=None, acceleration=1):
        """LZ4_compress_fast_continue over chains of linked blocks (lz4hip_compress_fast_chain_batch): chain c is the blocks
        chainFirst[c] .. chainFirst[c + 1] - 1, whose sources lie back to back from src[chainSrcOff[c]] on, behind chainPrefixLen[c]
        bytes of history that lie in front of it in src (None: no history; the stream loads it with LZ4_loadDict); block i owns the
        slot dst[dstOff[i]:+dstCap[i]] -> (outLen, chainConsumed): liblz4's return value per block (0: it did not fit, which ends
        the chain; CHAIN_STOPPED behind a chain's first 0) and the source bytes of each chain's blocks that succeeded (lists, or
        int32 / uint64 arrays for numpy inputs).  acceleration != 1: LZ4_compress_fast_continue's last argument for every block of
        the call (lz4hip_compress_fast_chain_accel_batch; clamped to 1 .. 65537 as liblz4 does)"""
        n, nc = cls._check_chains(src, chainSrcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainPrefixLen)
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        cons = (C.c_uint64 * max(nc, 1))()
        pre = _arr(C.c_int32, chainPrefixLen) if chainPrefixLen is not None else None
        args = (sp, _arr(C.c_uint64, chainSrcOff), pre, _arr(C.c_int32, srcLen), _arr(C.c_uint32, chainFirst), dp, _arr(C.c_uint64, dstOff),
                _arr(C.c_int32, dstCap), out, cons, n, nc)
        if acceleration == 1:
            _chk(lib().lz4hip_compress_fast_chain_batch(*args))
        else:
            _chk(lib().lz4hip_compress_fast_chain_accel_batch(*args, int(acceleration)))
        if hasattr(srcLen, "dtype"):
            import numpy as np
            return np.frombuffer(out, dtype=np.int32, count=n).copy(), np.frombuffer(cons, dtype=np.uint64, count=nc).copy()
        return list(out[:n]), list(cons[:nc])

    @classmethod
    def compressFastStream(cls, streams, streamId, src, chainSrcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainPrefixLen=None, acceleration=1):
        """LZ4_compress_fast_continue on streams that are continued from call to call (lz4hip_compress_fast_stream_batch): the arrays of
        compressFastChain, and chain c is the next run of blocks of stream streamId[c] of the CompressStreams set `streams` (ids
        strictly ascending).  For a stream that has run before, chainPrefixLen[c] is how many of the last bytes it consumed lie in front
        of the source (LZ4_saveDict's size; 0 is legal and no reset) -> (outLen, chainConsumed) as compressFastChain's; a block whose
        result is 0 stops its STREAM until it is reset.  acceleration != 1: LZ4_compress_fast_continue's last argument for every block
        of THIS call (lz4hip_compress_fast_stream_accel_batch); a stream may be given another one in every call"""
        n, nc = cls._check_chains(src, chainSrcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainPrefixLen)
        if len(streamId) != nc:
            raise ValueError("per-chain arrays differ in length")
        ns = len(streams)
        if hasattr(streamId, "dtype"):
            import numpy as np
            ids = np.asarray(streamId, dtype=np.int64)
            bad = nc and (ids[0] < 0 or ids[-1] >= ns or (np.diff(ids) <= 0).any())
        else:
            bad = any(streamId[c] < 0 or streamId[c] >= ns or (c and streamId[c] <= streamId[c - 1]) for c in range(nc))
        if bad:
            raise ValueError("streamId must be strictly ascending and below the number of streams")
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        cons = (C.c_uint64 * max(nc, 1))()
        pre = _arr(C.c_int32, chainPrefixLen) if chainPrefixLen is not None else None
        args = (streams._handle(), _arr(C.c_uint32, streamId), sp, _arr(C.c_uint64, chainSrcOff), pre, _arr(C.c_int32, srcLen), _arr(C.c_uint32, chainFirst),
                dp, _arr(C.c_uint64, dstOff), _arr(C.c_int32, dstCap), out, cons, n, nc)
        if acceleration == 1:
            _chk(lib().lz4hip_compress_fast_stream_batch(*args))
        else:
            _chk(lib().lz4hip_compress_fast_stream_accel_batch(*args, int(acceleration)))
        if hasattr(srcLen, "dtype"):
            import numpy as np
            return np.frombuffer(out, dtype=np.int32, count=n).copy(), np.frombuffer(cons, dtype=np.uint64, count=nc).copy()
        return list(out[:n]), list(cons[:nc])

    @classmethod
    def compressFastStreamAt(cls, streams, streamId, src, srcOff, srcLen, chainFirst, chainHistEnd, chainHistLen, chainWinOff, chainWinLen, dst, dstOff, dstCap,
                             acceleration=1):
        """The same streams when their sources land anywhere -- a ring that wraps, alternating buffers, a dictionary elsewhere
        (lz4hip_compress_fast_stream_ext_batch): every block has its own srcOff[i] inside its stream's window [chainWinOff[c],
        + chainWinLen[c]); the stream's history ends at chainHistEnd[c] in src with chainHistLen[c] bytes of it present.  A block that
        does not follow its history runs in liblz4's external-dictionary mode.  A call is a snapshot of src -> (outLen, chainConsumed)
        as compressFastStream's.  acceleration != 1: lz4hip_compress_fast_stream_ext_accel_batch, as for compressFastStream"""
        n, nc = len(srcLen), len(streamId)
        if not (len(srcOff) == len(dstOff) == len(dstCap) == n) or not (len(chainHistEnd) == len(chainHistLen) == len(chainWinOff) == len(chainWinLen) == nc) \
                or len(chainFirst) != nc + 1:
            raise ValueError("array lengths differ")
        ns = len(streams)
        if any(streamId[c] < 0 or streamId[c] >= ns or (c and streamId[c] <= streamId[c - 1]) for c in range(nc)):
            raise ValueError("streamId must be strictly ascending and below the number of streams")
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        cons = (C.c_uint64 * max(nc, 1))()
        args = (streams._handle(), _arr(C.c_uint32, streamId), sp, _arr(C.c_uint64, srcOff), _arr(C.c_int32, srcLen), _arr(C.c_uint32, chainFirst),
                _arr(C.c_uint64, chainHistEnd), _arr(C.c_int32, chainHistLen), _arr(C.c_uint64, chainWinOff), _arr(C.c_uint64, chainWinLen), dp,
                _arr(C.c_uint64, dstOff), _arr(C.c_int32, dstCap), out, cons, n, nc)
        if acceleration == 1:
            _chk(lib().lz4hip_compress_fast_stream_ext_batch(*args))
        else:
            _chk(lib().lz4hip_compress_fast_stream_ext_accel_batch(*args, int(acceleration)))
        if hasattr(srcLen, "dtype"):
            import numpy as np
            return np.frombuffer(out, dtype=np.int32, count=n).copy(), np.frombuffer(cons, dtype=np.uint64, count=nc).copy()
        return list(out[:n]), list(cons[:nc])

    @classmethod
    def decompressSafePartial(cls, src, srcOff, srcLen, dst, dstOff, targetLen, dstCap):
        """LZ4_decompress_safe_partial per block: the first min(targetLen[i], dstCap[i]) bytes of block i into the slot
        dst[dstOff[i]:+dstCap[i]] -> liblz4's return values (lz4hip_decompress_safe_partial_batch; lists, or an int32 array for numpy
        inputs); nothing is written past dstOff[i] + min(targetLen[i], dstCap[i])"""
        n = len(srcOff)
        if not (len(srcLen) == len(dstOff) == len(targetLen) == len(dstCap) == n):
            raise ValueError("per-block arrays differ in length")
        cls._check_ranges(src, srcOff, srcLen)
        cls._check_ranges(dst, dstOff, dstCap)
        sp, sk = _ro_ptr(src)
        dp, dk = _rw_ptr(dst)
        out = (C.c_int32 * max(n, 1))()
        _chk(lib().lz4hip_decompress_safe_partial_batch(sp, _arr(C.c_uint64, srcOff), _arr(C.c_int32, srcLen), dp, _arr(C.c_uint64, dstOff),
                                                        _arr(C.c_int32, targetLen), _arr(C.c_int32, dstCap), out, n))
        if hasattr(srcOff, "dtype"):
            import numpy as np
            return np.frombuffer(out, dtype=np.int32, count=n).copy()
        return list(out[:n])

    @classmethod
    def decompressedLengths(cls, src, srcOff, srcLen, maxDestLen):
        """what LZ4_decompress_safe would return per block -- the decoded size of src[srcOff[i]:+srcLen[i]] for a capacity of
        maxDestLen[i] bytes, or liblz4's negative code -- without any destination buffer (lz4hip_decompressed_size_batch; a list, or
        an int32 array for numpy inputs).  A result >= 0 means decompressSafe with that capacity succeeds and returns that number"""
        n = len(srcOff)
        if not (len(srcLen) == len(maxDestLen) == n):
            raise ValueError("per-block arrays differ in length")
        cls._check_ranges(src, srcOff, srcLen)
        for c in maxDestLen:
            _check_length(c)
        sp, sk = _ro_ptr(src)
        out = (C.c_int32 * max(n, 1))()
        _chk(lib().lz4hip_decompressed_size_batch(sp, _arr(C.c_uint64, srcOff), _arr(C.c_int32, srcLen), _arr(C.c_int32, maxDestLen), out, n))
        if hasattr(srcOff, "dtype"):
            import numpy as np
            return np.frombuffer(out, dtype=np.int32, count=n).copy()
        return list(out[:n])

    @classmethod
    def decompressSafeSized(cls, src, srcOff, srcLen, maxDestLen):
        """the batch twin of LZ4SafeDecompressor.decompress(src, maxDestLen) -> right-sized array: the sizes are queried first
        (decompressedLengths), a buffer of exactly sum(max(size, 0)) bytes is allocated with the blocks packed back to back, and
        every block that decodes is decoded into its slot.  Returns (buffer, offsets, lengths): lengths[i] is the decoded size, or
        liblz4's negative code for a block that does not decode with capacity maxDestLen[i] -- such a block has an empty slot.
        The worst-case n * maxDestLen bytes are never allocated"""
        sizes = [int(v) for v in cls.decompressedLengths(src, srcOff, srcLen, maxDestLen)]
        offsets, total = [], 0
        for v in sizes:
            offsets.append(total)
            total += max(v, 0)
        buf = bytearray(total)
        good = [i for i, v in enumerate(sizes) if v >= 0]
        if good:
            # every slot is decoded with its own size as the capacity.  liblz4 accepts a conforming block that way; a stream it
            # accepts only with room to spare (one that breaks the format's end rules, e.g. fewer than five last literals) comes
            # back with another value and is decoded once more, alone, through a scratch of its maxDestLen
            got = cls.decompressSafe(src, [srcOff[i] for i in good], [srcLen[i] for i in good], buf, [offsets[i] for i in good],
                                     [sizes[i] for i in good])
            for i, r in zip(good, got):
                if int(r) == sizes[i]:
                    continue
                scratch = bytearray(max(int(maxDestLen[i]), 1))
                r2 = cls.decompressSafe(src, [srcOff[i]], [srcLen[i]], scratch, [0], [int(maxDestLen[i])])[0]
                if int(r2) != sizes[i]:
                    raise LZ4HIPError("block %d: the decoder returned %d where the size query promised %d" % (i, int(r2), sizes[i]))
                buf[offsets[i]:offsets[i] + sizes[i]] = scratch[:sizes[i]]
        return buf, offsets, sizes

    @classmethod
    def xxh32(cls, buf, off, length, seed=0):
        n = len(off)
        if len(length) != n:
            raise ValueError("per-buffer arrays differ in length")
        cls._check_ranges(buf, off, length)
        p, k = _ro_ptr(buf)
        out = (C.c_uint32 * max(n, 1))()
        _chk(lib().lz4hip_xxh32_batch(p, _arr(C.c_uint64, off), _arr(C.c_int32, length), seed & 0xFFFFFFFF, out, n))
        return list(out[:n])

    @classmethod
    def xxh64(cls, buf, off, length, seed=0):
        n = len(off)
        if len(length) != n:
            raise ValueError("per-buffer arrays differ in length")
        cls._check_ranges(buf, off, length)
        p, k = _ro_ptr(buf)
        out = (C.c_uint64 * max(n, 1))()
        _chk(lib().lz4hip_xxh64_batch(p, _arr(C.c_uint64, off), _arr(C.c_int32, length), seed & 0xFFFFFFFFFFFFFFFF, out, n))
        return list(out[:n])


class CompressStreams:
    """A set of n compress streams whose state -- the hash table and index position an LZ4_stream_t carries beside its history -- is
    resident on the device between calls (lz4hip_cstreams_create): about 32 KB of device memory per stream.  Every stream gives, over
    all the calls that name it, the bytes ONE LZ4_stream_t of liblz4 gives, however its blocks are cut into calls.  Calls on one set
    are serialised.  close() -- or leaving a `with` block -- frees it, before lz4hip_shutdown()."""

    def __init__(self, n):
        self._h = C.c_void_p(None)
        if n < 1:
            raise ValueError("a set has at least one stream")
        _chk(lib().lz4hip_cstreams_create(int(n), C.byref(self._h)))

    def _handle(self):
        if not self._h:
            raise AssertionError("Already closed")
        return self._h

    def __len__(self):
        return lib().lz4hip_cstreams_count(self._handle())

    def compress(self, streamId, src, chainSrcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainPrefixLen=None, acceleration=1):
        """LZ4HIPBatch.compressFastStream on this set"""
        return LZ4HIPBatch.compressFastStream(self, streamId, src, chainSrcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainPrefixLen, acceleration)

    def compressAt(self, streamId, src, srcOff, srcLen, chainFirst, chainHistEnd, chainHistLen, chainWinOff, chainWinLen, dst, dstOff, dstCap, acceleration=1):
        """LZ4HIPBatch.compressFastStreamAt on this set: sources that land anywhere"""
        return LZ4HIPBatch.compressFastStreamAt(self, streamId, src, srcOff, srcLen, chainFirst, chainHistEnd, chainHistLen, chainWinOff, chainWinLen, dst, dstOff,
                                                dstCap, acceleration)

    def reset(self, streamId=None):
        """makes the listed streams (None: all of them) fresh"""
        if streamId is None:
            _chk(lib().lz4hip_cstreams_reset(self._handle(), None, 0))
        else:
            _chk(lib().lz4hip_cstreams_reset(self._handle(), _arr(C.c_uint32, streamId), len(streamId)))

    def consumed(self, first=0, n=None):
        """-> (bytes consumed since the reset, stopped) of the streams first .. first + n - 1, two lists"""
        n = len(self) - first if n is None else n
        cons = (C.c_uint64 * max(n, 1))()
        stop = (C.c_uint8 * max(n, 1))()
        _chk(lib().lz4hip_cstreams_consumed(self._handle(), first, n, cons, stop))
        return list(cons[:n]), [bool(v) for v in stop[:n]]

    def close(self):
        if self._h:
            lib().lz4hip_cstreams_free(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DecodeStreams:
    """The states of n decode streams -- per stream what an LZ4_streamDecode_t of liblz4 holds: (prefixEnd, prefixLen, extEnd, extLen) as
    offsets into the one destination buffer its caller decodes into.  Plain host data: there is nothing to close and nothing on a
    device.  Every stream gives, over all the calls that name it, the values and bytes ONE LZ4_streamDecode_t gives, however its
    blocks are cut into calls (LZ4HIPBatch.decompressSafeStream says when the bytes are liblz4's: the ring rule)."""

    def __init__(self, n, inOrder=False):
        """inOrder: the set's calls go to the in-order twin (LZ4HIPBatch.decompressSafeStream(inOrder=True)) unless a call says otherwise"""
        if n < 1:
            raise ValueError("a set has at least one stream")
        self._state = [(0, 0, 0, 0)] * int(n)
        self.inOrder = bool(inOrder)

    def __len__(self):
        return len(self._state)

    def set(self, streamId, prefixEnd, prefixLen):
        """LZ4_setStreamDecode: the stream starts behind the prefixLen bytes of dictionary that end at dst[prefixEnd]"""
        if prefixLen < 0 or prefixLen > prefixEnd:
            raise IndexError("history reaches in front of the buffer")
        self._state[streamId] = (int(prefixEnd), int(prefixLen), 0, 0)

    def reset(self, streamId=None):
        """makes the listed streams (None: all of them) fresh"""
        for c in (range(len(self._state)) if streamId is None else streamId):
            self._state[c] = (0, 0, 0, 0)

    def state(self, streamId=None):
        """-> the (prefixEnd, prefixLen, extEnd, extLen) of the listed streams (None: all of them)"""
        return [self._state[c] for c in (range(len(self._state)) if streamId is None else streamId)]

    def decompress(self, streamId, src, srcOff, srcLen, chainFirst, dst, dstOff, dstCap, chainWinOff, chainWinLen, inOrder=None):
        """LZ4HIPBatch.decompressSafeStream for the streams streamId (distinct ids, one per chain of the call) -> outLen.  inOrder: None =
        the set's own setting; the two entry points may alternate on a stream from call to call"""
        ids = [int(c) for c in streamId]
        if len(set(ids)) != len(ids):
            raise ValueError("a stream is named twice")
        out, new = LZ4HIPBatch.decompressSafeStream([self._state[c] for c in ids], src, srcOff, srcLen, chainFirst, dst, dstOff, dstCap,
                                                    chainWinOff, chainWinLen, inOrder=self.inOrder if inOrder is None else bool(inOrder))
        for c, s in zip(ids, new):
            self._state[c] = s
        return out


class CompressStreamsHC:
    """The states of n HC compress streams whose sources land anywhere -- per stream what an LZ4_streamHC_t of liblz4 keeps beside its
    tables: (prefixEnd, prefixLen, extEnd, extLen, index) as offsets into the one source buffer its caller compresses from.  Plain host
    data: there is nothing to close and nothing on a device.  Every stream gives, over all the calls that name it, the values and
    bytes ONE LZ4_streamHC_t gives, however its blocks are cut into calls (include/lz4hip.h states the exceptions)."""

    def __init__(self, n, level=9):
        if n < 1:
            raise ValueError("a set has at least one stream")
        self.level = int(level)
        self._state = [(0, 0, 0, 0, 0)] * int(n)

    def __len__(self):
        return len(self._state)

    def reset(self, streamId=None):
        """makes the listed streams (None: all of them) fresh"""
        for c in (range(len(self._state)) if streamId is None else streamId):
            self._state[c] = (0, 0, 0, 0, 0)

    def state(self, streamId=None):
        """-> the (prefixEnd, prefixLen, extEnd, extLen, index) of the listed streams (None: all of them)"""
        return [self._state[c] for c in (range(len(self._state)) if streamId is None else streamId)]

    def loadDict(self, streamId, dictEnd, dictLen):
        """LZ4_loadDictHC: the stream is fresh behind the dictLen bytes of dictionary that end at src[dictEnd]"""
        if dictLen < 0 or dictLen > dictEnd:
            raise IndexError("history reaches in front of the buffer")
        st = (C.c_uint64 * 5)()
        _chk(lib().lz4hip_hcstream_load_dict(st, int(dictEnd), int(dictLen)))
        self._state[streamId] = tuple(st)

    def saveDict(self, streamId, bufOff, k):
        """LZ4_saveDictHC for the caller who has copied the last k bytes the stream consumed to src[bufOff:] -> the bytes kept"""
        st = (C.c_uint64 * 5)(*self._state[streamId])
        kept = lib().lz4hip_hcstream_save_dict(st, int(bufOff), int(k))
        _chk(min(kept, 0))
        self._state[streamId] = tuple(st)
        return kept

    def compress(self, streamId, src, srcOff, srcLen, chainFirst, dst, dstOff, dstCap):
        """LZ4HIPBatch.compressHCStream at the set's level for the streams streamId (distinct ids, one per chain of the call) -> outLen"""
        ids = [int(c) for c in streamId]
        if len(set(ids)) != len(ids):
            raise ValueError("a stream is named twice")
        out, new = LZ4HIPBatch.compressHCStream([self._state[c] for c in ids], src, srcOff, srcLen, chainFirst, dst, dstOff, dstCap, self.level)
        for c, s in zip(ids, new):
            self._state[c] = s
        return out


# ----------------------------------------------------------------------------------------------
# device-resident batches (torch tensors are only the memory/stream plumbing)
# ----------------------------------------------------------------------------------------------
class DeviceBatch:
    """Device-pointer entry points on torch CUDA(HIP) tensors: uint8 data tensors, int64 offset
    tensors (reinterpreted as uint64), int32 length/capacity/result tensors.  Launches are enqueued
    on torch's current stream of the tensors' device and do not synchronise."""

    @staticmethod
    def _stream_dev(t):
        import torch
        return t.device.index or 0, torch.cuda.current_stream(t.device).cuda_stream

    @classmethod
    def _call(cls, fn, src, src_off, src_len, dst, dst_off, dst_cap, out):
        dev, st = cls._stream_dev(src)
        _chk(getattr(lib(), fn)(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(), dst_off.data_ptr(),
                                dst_cap.data_ptr(), out.data_ptr(), src_off.numel(), dev, st))

    @classmethod
    def compress_fast(cls, src, src_off, src_len, dst, dst_off, dst_cap, out, acceleration=1):
        """acceleration != 1: LZ4_compress_fast(..., acceleration) per block (lz4hip_compress_fast_accel_batch_dev)"""
        if acceleration == 1:
            cls._call("lz4hip_compress_fast_batch_dev", src, src_off, src_len, dst, dst_off, dst_cap, out)
            return
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_compress_fast_accel_batch_dev(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                        dst_off.data_ptr(), dst_cap.data_ptr(), out.data_ptr(), src_off.numel(),
                                                        int(acceleration), dev, st))

    @classmethod
    def compress_dest_size(cls, src, src_off, src_len, dst, dst_off, target_size, out, consumed):
        """LZ4_compress_destSize per block (lz4hip_compress_dest_size_batch_dev): out = bytes written, consumed = input consumed;
        block i's slot is dst[dst_off[i] : + target_size[i]]"""
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_compress_dest_size_batch_dev(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                       dst_off.data_ptr(), target_size.data_ptr(), out.data_ptr(), consumed.data_ptr(),
                                                       src_off.numel(), dev, st))

    @classmethod
    def compress_hc(cls, src, src_off, src_len, dst, dst_off, dst_cap, out, level=9):
        """asynchronous: the workspace is a torch tensor sized from the source tensor (an upper bound of the batch's source span);
        the caching allocator keeps it alive until the stream has used it"""
        import torch
        dev, st = cls._stream_dev(src)
        span = src.numel() * src.element_size()     # BYTES of the source tensor (the workspace holds one u16 per source byte)
        nb = lib().lz4hip_hc_workspace_bytes(span, src_off.numel(), level)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=src.device)
        _chk(lib().lz4hip_compress_hc_batch_dev_ws(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                   dst_off.data_ptr(), dst_cap.data_ptr(), out.data_ptr(), src_off.numel(), level, dev, st,
                                                   span, ws.data_ptr(), nb))
        ws.record_stream(torch.cuda.current_stream(src.device))

    @classmethod
    def compress_hc_dest_size(cls, src, src_off, src_len, dst, dst_off, target_size, out, consumed, level=9):
        """LZ4_compress_HC_destSize per block (lz4hip_compress_hc_dest_size_batch_dev_ws): out = bytes written, consumed = input
        consumed; block i's slot is dst[dst_off[i] : + target_size[i]].  Asynchronous, the workspace as in compress_hc"""
        import torch
        dev, st = cls._stream_dev(src)
        span = src.numel() * src.element_size()
        nb = lib().lz4hip_hc_workspace_bytes(span, src_off.numel(), level)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=src.device)
        _chk(lib().lz4hip_compress_hc_dest_size_batch_dev_ws(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                             dst_off.data_ptr(), target_size.data_ptr(), out.data_ptr(), consumed.data_ptr(),
                                                             src_off.numel(), level, dev, st, span, ws.data_ptr(), nb))
        ws.record_stream(torch.cuda.current_stream(src.device))

    @classmethod
    def compress_hc_dest_size_sync(cls, src, src_off, src_len, dst, dst_off, target_size, out, consumed, level=9):
        """the entry that sizes its own workspace (synchronises the stream once)"""
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_compress_hc_dest_size_batch_dev(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                          dst_off.data_ptr(), target_size.data_ptr(), out.data_ptr(), consumed.data_ptr(),
                                                          src_off.numel(), level, dev, st))

    @classmethod
    def container_blocks(cls, kind, src, block_size, dst, total, block_checksum=False, level=0):
        """device-resident container assembly, asynchronous on the current stream: src (uint8 tensor) cut into block_size pieces ->
        the LZ4 Frame (kind 0) / LZ4Block (kind 1) data blocks in dst; total = int64 tensor[1] receiving the bytes written (more
        than dst.numel(): the result is unusable)"""
        import torch
        dev, st = cls._stream_dev(src)
        nbytes = src.numel() * src.element_size()
        wsb = lib().lz4hip_container_workspace_bytes(nbytes, block_size, level)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=src.device)
        _chk(lib().lz4hip_container_blocks_dev(kind, 1 if block_checksum else 0, level, src.data_ptr(), nbytes, block_size, dst.data_ptr(),
                                               dst.numel() * dst.element_size(), total.data_ptr(), ws.data_ptr(), wsb, dev, st))
        ws.record_stream(torch.cuda.current_stream(src.device))

    @classmethod
    def compress_hc_sync(cls, src, src_off, src_len, dst, dst_off, dst_cap, out, level=9):
        """the entry that sizes its own workspace (synchronises the stream once)"""
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_compress_hc_batch_dev(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                dst_off.data_ptr(), dst_cap.data_ptr(), out.data_ptr(), src_off.numel(), level, dev, st))

    @classmethod
    def compress_fast_profile(cls, src, src_off, src_len, dst, dst_off, dst_cap, out, prof):
        """developer diagnostics: prof = int64 tensor [n, 12]"""
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_dbg_compress_fast_profile_dev(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                        dst_off.data_ptr(), dst_cap.data_ptr(), out.data_ptr(), src_off.numel(),
                                                        prof.data_ptr(), dev, st))

    @classmethod
    def decompress_safe(cls, src, src_off, src_len, dst, dst_off, dst_cap, out):
        cls._call("lz4hip_decompress_safe_batch_dev", src, src_off, src_len, dst, dst_off, dst_cap, out)

    @classmethod
    def decompress_fast(cls, src, src_off, src_cap, dst, dst_off, dst_len, out):
        cls._call("lz4hip_decompress_fast_batch_dev", src, src_off, src_cap, dst, dst_off, dst_len, out)

    @classmethod
    def compress_dict(cls, src, src_off, src_len, dst, dst_off, dst_cap, out, dictionary):
        """LZ4_loadDict + LZ4_compress_fast_continue per block, a fresh stream each (lz4hip_compress_fast_dict_batch_dev):
        `dictionary` is an LZ4Dictionary -- the handle, since the compressor needs its table image; out = compressed sizes, 0 where
        dst_cap[i] is too small.  Asynchronous, but a dictionary's first compress on a device waits for the stream once"""
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_compress_fast_dict_batch_dev(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                       dst_off.data_ptr(), dst_cap.data_ptr(), out.data_ptr(), src_off.numel(),
                                                       dictionary._handle(), dev, st))

    @classmethod
    def compress_hc_dict(cls, src, src_off, src_len, dst, dst_off, dst_cap, out, dictionary, level=9, span=None, ws=None):
        """LZ4_loadDictHC + LZ4_compress_HC_continue per block, a fresh stream each (lz4hip_compress_hc_dict_batch_dev_ws):
        `dictionary` is an LZ4Dictionary; out = compressed sizes, 0 where liblz4 returns 0.  The workspace as in compress_hc, or the
        caller's (span = the source bytes it is for, ws = a uint8 tensor).  Asynchronous, but a dictionary's first HC compress on a
        device waits for the stream once"""
        import torch
        dev, st = cls._stream_dev(src)
        if span is None:
            span = src.numel() * src.element_size()
        own = ws is None
        if own:
            ws = torch.empty(max(lib().lz4hip_hc_workspace_bytes(span, src_off.numel(), level), 1), dtype=torch.uint8, device=src.device)
        _chk(lib().lz4hip_compress_hc_dict_batch_dev_ws(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                        dst_off.data_ptr(), dst_cap.data_ptr(), out.data_ptr(), src_off.numel(), int(level),
                                                        dictionary._handle(), dev, st, span, ws.data_ptr(), ws.numel()))
        if own:
            ws.record_stream(torch.cuda.current_stream(src.device))

    @classmethod
    def compress_hc_dict_sync(cls, src, src_off, src_len, dst, dst_off, dst_cap, out, dictionary, level=9):
        """the entry that sizes its own workspace (lz4hip_compress_hc_dict_batch_dev; synchronises the stream once)"""
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_compress_hc_dict_batch_dev(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                     dst_off.data_ptr(), dst_cap.data_ptr(), out.data_ptr(), src_off.numel(), int(level),
                                                     dictionary._handle(), dev, st))

    @classmethod
    def decompress_safe_dict(cls, src, src_off, src_len, dst, dst_off, dst_cap, out, dictionary):
        """LZ4_decompress_safe_usingDict per block (lz4hip_decompress_safe_dict_batch_dev): `dictionary` is a uint8 tensor on the
        blocks' device holding the whole dictionary (or its last 64 KB or more); out = liblz4's return values.  The tensor must stay
        alive until the work on the stream is done"""
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_decompress_safe_dict_batch_dev(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                         dst_off.data_ptr(), dst_cap.data_ptr(), out.data_ptr(), src_off.numel(),
                                                         dictionary.data_ptr() if dictionary.numel() else None, dictionary.numel(),
                                                         dev, st))

    @classmethod
    def decompress_safe_chain(cls, src, src_off, src_len, dst_cap, chain_first, dst, chain_dst_off, chain_dst_cap, out, chain_out,
                              chain_prefix_len=None, stored=None):
        """LZ4_decompress_safe_continue over chains of linked blocks (lz4hip_decompress_safe_chain_batch_dev): chain_first is an int32
        tensor of chains + 1 entries (reinterpreted as uint32), chain_dst_off / chain_dst_cap / chain_out int64 tensors (as uint64),
        chain_prefix_len an int32 tensor or None, stored a uint8 tensor or None; out = liblz4's return values per block
        (LZ4HIPBatch.CHAIN_STOPPED behind a chain's first negative one), chain_out = the bytes each chain decoded"""
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_decompress_safe_chain_batch_dev(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(),
                                                          stored.data_ptr() if stored is not None else None, dst_cap.data_ptr(),
                                                          chain_first.data_ptr(), dst.data_ptr(), chain_dst_off.data_ptr(), chain_dst_cap.data_ptr(),
                                                          chain_prefix_len.data_ptr() if chain_prefix_len is not None else None,
                                                          out.data_ptr(), chain_out.data_ptr(), src_off.numel(), chain_dst_off.numel(), dev, st))

    @classmethod
    def compress_fast_chain(cls, src, chain_src_off, src_len, chain_first, dst, dst_off, dst_cap, out, chain_consumed, chain_prefix_len=None):
        """LZ4_compress_fast_continue over chains of linked blocks (lz4hip_compress_fast_chain_batch_dev): chain_first is an int32
        tensor of chains + 1 entries (reinterpreted as uint32), chain_src_off / dst_off / chain_consumed int64 tensors (as uint64),
        chain_prefix_len an int32 tensor or None; out = liblz4's return values per block (0 ends a chain, LZ4HIPBatch.CHAIN_STOPPED
        behind it), chain_consumed = the source bytes of each chain's blocks that succeeded"""
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_compress_fast_chain_batch_dev(src.data_ptr(), chain_src_off.data_ptr(),
                                                        chain_prefix_len.data_ptr() if chain_prefix_len is not None else None,
                                                        src_len.data_ptr(), chain_first.data_ptr(), dst.data_ptr(), dst_off.data_ptr(),
                                                        dst_cap.data_ptr(), out.data_ptr(), chain_consumed.data_ptr(), src_len.numel(),
                                                        chain_src_off.numel(), dev, st))

    @classmethod
    def decompress_safe_partial(cls, src, src_off, src_len, dst, dst_off, target_len, dst_cap, out):
        """LZ4_decompress_safe_partial per block (lz4hip_decompress_safe_partial_batch_dev): out = liblz4's return values; block i
        decodes into min(target_len[i], dst_cap[i]) bytes of its slot dst[dst_off[i] : + dst_cap[i]]"""
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_decompress_safe_partial_batch_dev(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst.data_ptr(),
                                                            dst_off.data_ptr(), target_len.data_ptr(), dst_cap.data_ptr(), out.data_ptr(),
                                                            src_off.numel(), dev, st))

    @classmethod
    def decoded_size(cls, src, src_off, src_len, dst_cap, out):
        """the decoded-size query (lz4hip_decompressed_size_batch_dev): out[i] = what decompress_safe would return for block i with
        capacity dst_cap[i]; there is no destination tensor and nothing but out is written"""
        dev, st = cls._stream_dev(src)
        _chk(lib().lz4hip_decompressed_size_batch_dev(src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), dst_cap.data_ptr(),
                                                      out.data_ptr(), src_off.numel(), dev, st))

    @classmethod
    def xxh32(cls, buf, off, length, seed, out):
        dev, st = cls._stream_dev(buf)
        _chk(lib().lz4hip_xxh32_batch_dev(buf.data_ptr(), off.data_ptr(), length.data_ptr(), seed & 0xFFFFFFFF, out.data_ptr(),
                                          off.numel(), dev, st))

    @classmethod
    def xxh64(cls, buf, off, length, seed, out):
        dev, st = cls._stream_dev(buf)
        _chk(lib().lz4hip_xxh64_batch_dev(buf.data_ptr(), off.data_ptr(), length.data_ptr(), seed & 0xFFFFFFFFFFFFFFFF,
                                          out.data_ptr(), off.numel(), dev, st))

    @classmethod
    def gen_blocks(cls, dst, stride, block_len, n_blocks, first_idx=0, seed=0x4C5A3447, litmax=38, win=65535):
        dev, st = cls._stream_dev(dst)
        _chk(lib().lz4hip_gen_blocks_dev(dst.data_ptr(), stride, block_len, seed, first_idx, litmax, win, n_blocks, dev, st))


def decoderRingBufferSize(maxBlock):
    """LZ4_decoderRingBufferSize: the smallest ring a stream of blocks of up to maxBlock bytes is decoded into (DecodeStreams(inOrder=True));
    0 for a negative maxBlock or one above 0x7E000000"""
    return int(lib().lz4hip_decoder_ring_buffer_size(int(maxBlock)))


def set_option(name, value):
    """a tuning knob of include/lz4hip.h: "decode_stage", "decode_pipe", "decode_route_short", "decode_route_slots" (1 .. 256 of the route
    ring's slots handed out), "decode_ring", "decode_lanes", "compress_core", "compress_pack", "hc_chain_segment", "compress_switch", "dstream_inorder"
    (1: every block of decompressSafeStream(inOrder=True) goes through the in-order tier, not only those whose slots overlap).  Every
    setting produces the same bytes; an unknown name or a value outside the knob's range raises LZ4HIPError"""
    _chk(lib().lz4hip_set_option(name.encode(), value))


def last_decode_route(device=0):
    """diagnostic: (route, sampled hops, sampled stream bytes, average compressed size, sampled offsets within 6 KB, sampled sequences,
    their output bytes, 0) of the last decode launch that was routed on the device (more than 16 blocks per compute unit, every knob at
    its default); route 0 = lane-group default of the batch size, 1 = ring loop, 2 = wave loop, 3 = deep loop instead of the staged one.
    The last routed launch on WHICHEVER stream it ran: a single-stream diagnostic"""
    out = (C.c_uint32 * 8)()
    _chk(lib().lz4hip_last_decode_route(device, out))
    return tuple(int(x) for x in out)
