#!/usr/bin/env python3
"""tools/dstream_sweep.py -- what the stream decoder's state machine costs (lz4hip_decompress_safe_stream_batch, decode_stream_kernel)
beside the chain decoder (lz4hip_decompress_safe_chain_batch, decode_chain_kernel) on one MI355X.

Both entry points take host pointers, so wall time is staging; what is compared is KERNEL time.  Every cell runs in a child process of
its own under `rocprofv3 --kernel-trace --stats` (nothing else is collected in that run), and the kernels' total times are read from
the child's kernel-stats table.  A cell is N streams of 16 x 4 KiB blocks, written by the reference library's
LZ4_compress_fast_continue (one LZ4_stream_t per stream over contiguous data), decoded in ONE call each by
  chain     decode_chain_kernel: the blocks back to back
  stream a  decode_stream_kernel, layout a: the same destinations, from a fresh state -- the chain kernel's loops plus a state record
  stream d  decode_stream_kernel, layout d: a ring of 65535 + 2 x 4096 bytes entered at offset 40000, so that the ninth block wraps to 0:
            eight blocks on the rolling prefix, one after the jump (forceExtDict), seven while the new prefix grows behind the old one
            (doubleDict)
on Calgary book1 (tests/golden/calgary/book1.xz) and the App. F synthetic blocks (oracle.gen_block); a pool of 512 distinct streams is
tiled to the cell's stream count.  The child also checks that all three give the same results and, on a sample, the writer's bytes.

  python tools/dstream_sweep.py [--streams 65536,4096] [--data appf,book1] [--out profiles/dstream_sweep.txt]
"""
import argparse
import csv
import ctypes as C
import glob
import importlib
import lzma
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK, BLOCKS = 4096, 16
RING, ENTER = 65535 + 2 * BLOCK, 40000


def worker(kind, n):
    """one cell, no timing of its own: the chain call, then the two stream calls; prints `cell ok <decoded bytes>`"""
    import numpy as np
    amd = importlib.import_module("lz4-java_amd")
    from oracle import oracle as O
    L = C.CDLL(O.ref().path)
    L.LZ4_createStream.restype = C.c_void_p
    L.LZ4_freeStream.argtypes = [C.c_void_p]
    L.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    book = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "calgary", "book1.xz"), "rb").read())
    stride = BLOCK * BLOCKS
    pool = min(512, n)
    def raw(k):
        if kind == "book1":
            o = (k * 104729) % (len(book) - stride)
            return book[o:o + stride]
        return O.gen_block(stride, 1000 + k)
    raws, comp, lens = [], bytearray(), []
    for k in range(pool):
        r = raw(k)
        raws.append(r)
        buf = C.create_string_buffer(r, stride)
        st = L.LZ4_createStream()
        for i in range(BLOCKS):
            dst = C.create_string_buffer(BLOCK + BLOCK // 255 + 32)
            m = L.LZ4_compress_fast_continue(st, C.addressof(buf) + i * BLOCK, dst, BLOCK, len(dst), 1)
            assert m > 0
            comp += dst.raw[:m]; lens.append(m)
        L.LZ4_freeStream(st)
    reps = (n + pool - 1) // pool
    src = np.tile(np.frombuffer(bytes(comp), dtype=np.uint8), reps)
    src_len = np.tile(np.array(lens, dtype=np.int32), reps)[:n * BLOCKS]
    src_off = np.concatenate([[0], np.cumsum(src_len.astype(np.uint64))[:-1]]).astype(np.uint64)
    first = np.arange(n + 1, dtype=np.uint32) * np.uint32(BLOCKS)
    cap = np.full(n * BLOCKS, BLOCK, np.int32)
    sample = list(range(0, n, max(1, n // 64)))
    # chain, and stream layout a: windows of 16 blocks, back to back
    win_off = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    win_len = np.full(n, stride, np.uint64)
    dst = np.zeros(n * stride, np.uint8)
    c_out, c_len = amd.LZ4HIPBatch.decompressSafeChain(src, src_off, src_len, cap, first, dst, win_off, win_len)
    assert (c_out == BLOCK).all() and (c_len == stride).all()
    for c in sample:
        assert dst[c * stride:(c + 1) * stride].tobytes() == raws[c % pool], "the chain call's bytes"
    dst[:] = 0
    dst_off = (np.arange(n * BLOCKS, dtype=np.uint64) * np.uint64(BLOCK))
    a_out, a_state = amd.LZ4HIPBatch.decompressSafeStream([(0, 0, 0, 0)] * n, src, src_off, src_len, first, dst, dst_off, cap, win_off, win_len)
    assert (a_out == c_out).all() and all(s[1] == stride for s in a_state)
    for c in sample:
        assert dst[c * stride:(c + 1) * stride].tobytes() == raws[c % pool], "layout a's bytes"
    del dst
    # stream layout d: a ring per stream, entered at ENTER
    pos, p = [], ENTER
    for i in range(BLOCKS):
        if p + BLOCK > RING:
            p = 0
        pos.append(p); p += BLOCK
    assert pos[8] == 0
    ring = np.zeros(n * RING, np.uint8)
    win_off = np.arange(n, dtype=np.uint64) * np.uint64(RING)
    win_len = np.full(n, RING, np.uint64)
    dst_off = (win_off[:, None] + np.array(pos, dtype=np.uint64)[None, :]).reshape(-1)
    d_out, d_state = amd.LZ4HIPBatch.decompressSafeStream([(0, 0, 0, 0)] * n, src, src_off, src_len, first, ring, dst_off, cap, win_off, win_len)
    assert (d_out == c_out).all() and all(s[1] == 8 * BLOCK and s[3] == 8 * BLOCK for s in d_state)
    for c in sample:
        got = b"".join(ring[c * RING + q:c * RING + q + BLOCK].tobytes() for q in pos)
        assert got == raws[c % pool], "layout d's bytes"
    print("cell ok %d" % (n * stride), flush=True)


def kernel_ns(d):
    """{kernel name: (calls, total ns)} of the kernel-stats table rocprofv3 left under d"""
    res = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(p) as fh:
            for row in csv.DictReader(fh):
                col = lambda *w: next(v for k, v in row.items() if all(x in k.lower() for x in w))
                res[col("name")] = (int(col("calls")), int(float(col("total"))))
    return res


def trace_ns(d, name):
    """the kernel's launches in order of their start, from the kernel trace: [ns per launch]"""
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(p) as fh:
            for row in csv.DictReader(fh):
                col = lambda *w: next(v for k, v in row.items() if all(x in k.lower() for x in w))
                if name in col("kernel", "name"):
                    rows.append((int(col("start")), int(col("end")) - int(col("start"))))
    return [t for _, t in sorted(rows)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="65536,4096")
    ap.add_argument("--data", default="appf,book1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--work", default=None, help="directory for the profiler's output of every cell (default: beside --out, else the current directory)")
    ap.add_argument("--cell-timeout", type=int, default=420)
    ap.add_argument("--worker", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], int(args.worker[1]))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# dstream_sweep: kernel time of decode_stream_kernel (N streams x 16 blocks of 4 KiB in ONE call; layout a: back to back, layout d: a")
    emit("# ring of %d bytes entered at %d) beside decode_chain_kernel on the same streams; rocprofv3 --kernel-trace --stats, one run per cell" % (RING, ENTER))
    emit("%6s %8s %12s %12s %12s %11s %11s %11s %8s %8s" % ("data", "streams", "chain ms", "stream a ms", "stream d ms", "chain GB/s", "a GB/s", "d GB/s", "a/chain", "d/chain"))
    work = args.work or (os.path.dirname(os.path.abspath(args.out)) if args.out else os.getcwd())
    os.makedirs(work, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="dstream_sweep_", dir=work)
    stop = False
    for kind in args.data.split(","):
        for n in (int(v) for v in args.streams.split(",")):
            d = os.path.join(tmp, "%s_%d" % (kind, n))
            # (timeout -k: the profiler AND the worker behind it end with the time limit; start_new_session + killpg below: nothing of the
            # cell outlives it, whatever ended it)
            cmd = ["timeout", "-k", "10", str(args.cell_timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--worker", kind, str(n)]
            p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
            try:
                so, se = p.communicate(timeout=args.cell_timeout + 30)
                status, tail = p.returncode, (se or so)[-300:].replace("\n", " | ")
                good = status == 0 and "cell ok" in so
            except subprocess.TimeoutExpired:
                status, tail, good = 124, "time limit", False
            finally:
                try:
                    os.killpg(p.pid, signal.SIGKILL)   # (the group is gone after a clean end: nothing to do then)
                except (ProcessLookupError, PermissionError):
                    pass
                if p.poll() is None:
                    p.wait()
            if not good:   # (whatever ended it: nothing more is started on the device after a run that failed)
                emit("# %s %d: the cell's run failed (status %d): %s" % (kind, n, status, tail))
                emit("# stopping here")
                stop = True
                break
            ks = kernel_ns(d)
            ch = [v for k, v in ks.items() if "decode_chain_kernel" in k]
            st = trace_ns(d, "decode_stream_kernel")
            if not ch or len(st) < 2 or len(st) % 2:
                emit("# %s %d: no usable kernel rows (%d stats rows, %d stream launches)" % (kind, n, len(ks), len(st)))
                continue
            # (the host path cuts a call into chunks, each a launch: the first half of the stream kernel's launches is layout a's call)
            c_ns, a_ns, d_ns = ch[0][1], sum(st[:len(st) // 2]), sum(st[len(st) // 2:])
            total = float(n) * BLOCK * BLOCKS
            emit("%6s %8d %12.3f %12.3f %12.3f %11.2f %11.2f %11.2f %8.3f %8.3f"
                 % (kind, n, c_ns / 1e6, a_ns / 1e6, d_ns / 1e6, total / c_ns, total / a_ns, total / d_ns, a_ns / c_ns, d_ns / c_ns))
            shutil.rmtree(d, ignore_errors=True)
        if stop:
            break
    emit("# ms = total kernel time of the call's launches (the host path cuts a call into chunks of 64 MiB of compressed bytes or 512 MiB of")
    emit("# device image, each a launch); GB/s = decoded bytes / kernel time; a/chain, d/chain = stream / chain kernel time.  The chain kernel is")
    emit("# instruction-identical to the parent's (profiles/dstream_kernel_diff.txt).  %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
