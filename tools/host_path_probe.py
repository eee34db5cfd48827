#!/usr/bin/env python3
"""Host-pointer batch API on headline blocks in pageable host memory: GB/s per call (PCIe both ways) and, with
LZ4HIP_HOST_PROF=1 in the environment, the calling thread's time split per call (stderr).  Per call: the block path
(lz4hip_compress_fast_batch, lz4hip_decompress_safe_batch on n_blocks x 64 KiB), the chain paths
(lz4hip_compress_fast_chain_batch, lz4hip_decompress_safe_chain_batch on `chains` chains of 16 x 4 KiB: the first bytes of the
same data), the hash path (lz4hip_xxh64_batch on the n_blocks x 64 KiB) and, on the same chains, the other entries whose unit is a
chain or a stream: lz4hip_decompress_safe_stream_batch (fresh states, a stream's window = its chain's region),
lz4hip_compress_hc_chain_batch (level 9), lz4hip_compress_hc_stream_batch (zero states, blocks back to back, level 9) and
lz4hip_compress_fast_stream_batch / lz4hip_compress_fast_stream_ext_batch on a set of `chains` resident streams, reset between calls.
Every compressed result is decoded again (lz4hip_decompress_safe_chain_batch, not timed) and compared.  GB/s counts uncompressed bytes.
usage: host_path_probe.py [n_blocks=16384] [calls=4] [chains=4096]"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
amd = importlib.import_module("lz4-java_amd")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 4
nc = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
blk = 65536; cap = amd.maxCompressedLength(blk)
per, cblk = 16, 4096; ccap = amd.maxCompressedLength(cblk)   # a chain: 16 blocks of 4 KiB, 64 KiB of source
nc = min(nc, n)
dev = torch.device("cuda:0")
src = torch.empty(n * blk, dtype=torch.uint8, device=dev); amd.DeviceBatch.gen_blocks(src, blk, blk, n)
h_src = src.cpu().numpy().copy()
del src
so = np.arange(n, dtype=np.uint64) * blk; sl = np.full(n, blk, dtype=np.int32)
co = np.arange(n, dtype=np.uint64) * cap; cc = np.full(n, cap, dtype=np.int32)
h_dst = np.zeros(n * cap, dtype=np.uint8); h_back = np.zeros(n * blk, dtype=np.uint8)
clen = np.zeros(n, dtype=np.int32); dlen = np.zeros(n, dtype=np.int32)
# the chains: chain c is the 64 KiB at c * 65536 of the same source, its blocks' slots back to back in k_dst
nb = nc * per
k_so = np.arange(nc, dtype=np.uint64) * (per * cblk); k_sl = np.full(nb, cblk, dtype=np.int32)
k_first = (np.arange(nc + 1, dtype=np.uint32) * per).astype(np.uint32)
k_do = np.arange(nb, dtype=np.uint64) * ccap; k_dc = np.full(nb, ccap, dtype=np.int32)
k_dst = np.zeros(nb * ccap, dtype=np.uint8); k_back = np.zeros(nb * cblk, dtype=np.uint8)
k_out = np.zeros(nb, dtype=np.int32); k_cons = np.zeros(nc, dtype=np.uint64)
k_cap = np.full(nc, per * cblk, dtype=np.uint64); k_dlen = np.zeros(nb, dtype=np.int32); k_done = np.zeros(nc, dtype=np.uint64)
hashes = np.zeros(n, dtype=np.uint64)
# the stream forms of the same chains: per-block source offsets, a window per stream, state records, a set of nc resident streams
b_so = np.arange(nb, dtype=np.uint64) * cblk
ids = np.arange(nc, dtype=np.uint32); no_hist = np.zeros(nc, dtype=np.int32)
x_dst = np.zeros(nb * ccap, dtype=np.uint8); x_out = np.zeros(nb, dtype=np.int32); x_cons = np.zeros(nc, dtype=np.uint64)
d_state = np.zeros(4 * nc, dtype=np.uint64); hc_state = np.zeros(5 * nc, dtype=np.uint64)
HC_LEVEL = 9
import ctypes as C
lib = amd.lib()
def p(a):
    t = {np.uint64: C.POINTER(C.c_uint64), np.int32: C.POINTER(C.c_int32), np.uint32: C.POINTER(C.c_uint32)}.get(a.dtype.type)
    return a.ctypes.data_as(t) if t else a.ctypes.data_as(C.c_void_p)
def timed(f, *a):
    t0 = time.perf_counter()
    rc = f(*a)
    dt = time.perf_counter() - t0
    assert rc == 0, (rc, lib.lz4hip_last_error())
    return dt
streams = C.c_void_p(None)
assert lib.lz4hip_cstreams_create(nc, C.byref(streams)) == 0, lib.lz4hip_last_error()
def round_trip(dst, out):
    """what a chain compressor left in (dst, out), back through lz4hip_decompress_safe_chain_batch: the chains' bytes again?"""
    k_back[:] = 0
    rc = lib.lz4hip_decompress_safe_chain_batch(p(dst), p(k_do), p(out), None, p(k_sl), p(k_first), p(k_back), p(k_so), p(k_cap), None, p(k_dlen), p(k_done), nb, nc)
    return rc == 0 and bool((k_back == h_src[:nb * cblk]).all() and (k_dlen == cblk).all() and (k_done == per * cblk).all())
for c in range(calls):
    t_c = timed(lib.lz4hip_compress_fast_batch, p(h_src), p(so), p(sl), p(h_dst), p(co), p(cc), p(clen), n)
    t_d = timed(lib.lz4hip_decompress_safe_batch, p(h_dst), p(co), p(clen), p(h_back), p(so), p(sl), p(dlen), n)
    print("call %d: compress %.1f ms (%.1f GB/s)  decompress %.1f ms (%.1f GB/s)  ok=%s" % (
        c, 1e3 * t_c, n * blk / t_c / 1e9, 1e3 * t_d, n * blk / t_d / 1e9, bool((h_back == h_src).all() and (dlen == blk).all())), flush=True)
    t_kc = timed(lib.lz4hip_compress_fast_chain_batch, p(h_src), p(k_so), None, p(k_sl), p(k_first), p(k_dst), p(k_do), p(k_dc), p(k_out), p(k_cons), nb, nc)
    t_kd = timed(lib.lz4hip_decompress_safe_chain_batch, p(k_dst), p(k_do), p(k_out), None, p(k_sl), p(k_first), p(k_back), p(k_so), p(k_cap), None,
                 p(k_dlen), p(k_done), nb, nc)
    t_h = timed(lib.lz4hip_xxh64_batch, p(h_src), p(so), p(sl), 0, p(hashes), n)
    ok = bool((k_back == h_src[:nb * cblk]).all() and (k_dlen == cblk).all() and (k_cons == per * cblk).all() and (k_done == per * cblk).all())
    print("call %d: chain compress %.1f ms (%.1f GB/s)  chain decompress %.1f ms (%.1f GB/s)  xxh64 %.1f ms (%.1f GB/s)  ok=%s" % (
        c, 1e3 * t_kc, nb * cblk / t_kc / 1e9, 1e3 * t_kd, nb * cblk / t_kd / 1e9, 1e3 * t_h, n * blk / t_h / 1e9, ok), flush=True)
    d_state[:] = 0; k_back[:] = 0
    t_sd = timed(lib.lz4hip_decompress_safe_stream_batch, p(d_state), p(k_dst), p(k_do), p(k_out), p(k_first), p(k_back), p(b_so), p(k_sl), p(k_so), p(k_cap), p(k_dlen), nb, nc)
    ok = bool((k_back == h_src[:nb * cblk]).all() and (k_dlen == cblk).all())
    t_hc = timed(lib.lz4hip_compress_hc_chain_batch, p(h_src), p(k_so), None, p(k_sl), p(k_first), p(x_dst), p(k_do), p(k_dc), p(x_out), nb, nc, HC_LEVEL)
    ok = round_trip(x_dst, x_out) and ok
    hc_state[:] = 0
    t_hs = timed(lib.lz4hip_compress_hc_stream_batch, p(hc_state), p(h_src), p(b_so), p(k_sl), p(k_first), p(x_dst), p(k_do), p(k_dc), p(x_out), nb, nc, HC_LEVEL)
    ok = round_trip(x_dst, x_out) and ok
    print("call %d: stream decompress %.1f ms (%.1f GB/s)  hc chain compress %.1f ms (%.1f GB/s)  hc stream compress %.1f ms (%.1f GB/s)  ok=%s" % (
        c, 1e3 * t_sd, nb * cblk / t_sd / 1e9, 1e3 * t_hc, nb * cblk / t_hc / 1e9, 1e3 * t_hs, nb * cblk / t_hs / 1e9, ok), flush=True)
    assert lib.lz4hip_cstreams_reset(streams, None, 0) == 0, lib.lz4hip_last_error()
    x_cons[:] = 0
    t_fs = timed(lib.lz4hip_compress_fast_stream_batch, streams, p(ids), p(h_src), p(k_so), None, p(k_sl), p(k_first), p(x_dst), p(k_do), p(k_dc), p(x_out), p(x_cons), nb, nc)
    ok = round_trip(x_dst, x_out) and bool((x_cons == per * cblk).all())
    assert lib.lz4hip_cstreams_reset(streams, None, 0) == 0, lib.lz4hip_last_error()
    x_cons[:] = 0
    t_fx = timed(lib.lz4hip_compress_fast_stream_ext_batch, streams, p(ids), p(h_src), p(b_so), p(k_sl), p(k_first), p(k_so), p(no_hist), p(k_so), p(k_cap), p(x_dst), p(k_do),
                 p(k_dc), p(x_out), p(x_cons), nb, nc)
    ok = round_trip(x_dst, x_out) and bool((x_cons == per * cblk).all()) and ok
    print("call %d: stream compress %.1f ms (%.1f GB/s)  stream ext compress %.1f ms (%.1f GB/s)  ok=%s" % (
        c, 1e3 * t_fs, nb * cblk / t_fs / 1e9, 1e3 * t_fx, nb * cblk / t_fx / 1e9, ok), flush=True)
lib.lz4hip_cstreams_free(streams)
