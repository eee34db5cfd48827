#!/usr/bin/env python3
"""tools/cxstream_sweep.py -- what the walk for sources that land anywhere costs (lz4hip_compress_fast_stream_ext_batch,
compress_fast_xstream_cu_kernel) on one MI355X, and what a history of one block costs in output size.

The entry points take host pointers, so wall time is staging; what is compared is KERNEL time.  Every cell runs in a child process of
its own under `rocprofv3 --kernel-trace --stats` (nothing else is collected in that run).  A cell is N streams of 16 x 4 KiB blocks, in
ONE call or in 16 calls of one block, through
  stream   compress_fast_stream_cu_kernel (lz4hip_compress_fast_stream_batch), the blocks back to back -- the kernel the parent commit
           has, instruction for instruction (profiles/xstream_kernel_diff.txt)
  ext a    compress_fast_xstream_cu_kernel on the same blocks back to back: every block in prefix mode, so ext a / stream is the new
           walk's overhead
  ext b    compress_fast_xstream_cu_kernel with one block of history: in 16 calls the producer's two alternating buffers of 4096 bytes;
           in ONE call -- a call is a snapshot, two buffers hold two blocks -- every block in a place of its own, 64 bytes behind the
           block before it: every block jumps and sees the block before it, the same history (not the same bytes: on two ADJACENT
           buffers every other block follows its history and runs in prefix mode)
  cpu      the reference library's LZ4_compress_fast_continue on the two alternating buffers on 16 host threads
           (tools/cxstream_refbench.c), wall time
on Calgary book1 (tests/golden/calgary/book1.xz) and the App. F synthetic blocks (oracle.gen_block); a pool of 512 distinct streams is
tiled to the cell's stream count.  The child checks ext a's sizes against stream's and a sample of ext b's bytes against the reference.

  python tools/cxstream_sweep.py [--streams 65536,4096] [--data appf,book1] [--calls 1,16] [--out profiles/cxstream_sweep.txt]
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
BLOCK, BLOCKS, GAP = 4096, 16, 64


def pool_streams(kind, pool):
    from oracle import oracle as O
    book = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "calgary", "book1.xz"), "rb").read())
    stride = BLOCK * BLOCKS
    def raw(k):
        if kind == "book1":
            o = (k * 104729) % (len(book) - stride)
            return book[o:o + stride]
        return O.gen_block(stride, 1000 + k)
    return [raw(k) for k in range(pool)]


def worker(kind, n, calls):
    """one cell, no timing of its own: stream, ext a, a marker launch, ext b; prints `cell ok <ext a bytes> <ext b bytes>`"""
    import numpy as np
    amd = importlib.import_module("lz4-java_amd")
    from oracle import oracle as O
    stride = BLOCK * BLOCKS
    pool = min(512, n)
    raws = pool_streams(kind, pool)
    one = np.frombuffer(b"".join(raws), dtype=np.uint8)
    src = np.tile(one, (n + pool - 1) // pool)[:n * stride]
    blocks = src.reshape(n, BLOCKS, BLOCK)
    cap = BLOCK + BLOCK // 255 + 16
    per = BLOCKS // calls
    ids = np.arange(n, dtype=np.uint32)
    base = np.arange(n, dtype=np.int64) * stride
    dst = np.zeros(n * BLOCKS * cap, np.uint8)
    first = np.arange(n + 1, dtype=np.uint32) * np.uint32(per)
    sl = np.full(n * per, BLOCK, np.int32)
    dc = np.full(n * per, cap, np.int32)
    slots = lambda k: ((np.arange(n, dtype=np.int64)[:, None] * BLOCKS + np.arange(k * per, (k + 1) * per, dtype=np.int64)[None, :]).reshape(-1)) * cap
    # stream: the existing entry, the data left in place
    s_out = np.zeros((n, BLOCKS), np.int32)
    with amd.CompressStreams(n) as streams:
        for k in range(calls):
            done = k * per * BLOCK
            out, cons = streams.compress(ids, src, base + done, sl, first, dst, slots(k), dc, np.full(n, done, np.int32))
            assert int(cons.sum()) == n * per * BLOCK, "a stream of the cell stopped"
            s_out[:, k * per:(k + 1) * per] = out.reshape(n, per)
    # ext a: the same blocks, the same places
    a_out = np.zeros((n, BLOCKS), np.int32)
    with amd.CompressStreams(n) as streams:
        for k in range(calls):
            done = k * per * BLOCK
            so = (base[:, None] + done + np.arange(per, dtype=np.int64)[None, :] * BLOCK).reshape(-1)
            out, cons = streams.compressAt(ids, src, so, sl, first, base + done, np.full(n, min(done, 65536), np.int32), base, np.full(n, stride, np.int64),
                                           dst, slots(k), dc)
            assert int(cons.sum()) == n * per * BLOCK
            a_out[:, k * per:(k + 1) * per] = out.reshape(n, per)
    assert (a_out == s_out).all(), "ext a's sizes differ from the stream call's"
    # a marker between the two halves of the new kernel's launches: one tiny chain through the chain kernel
    amd.LZ4HIPBatch.compressFastChain(bytes(64), [0], [64], [0, 1], bytearray(128), [0], [128])
    # ext b: one block of history
    b_out = np.zeros((n, BLOCKS), np.int32)
    with amd.CompressStreams(n) as streams:
        if calls == 1:
            w = BLOCKS * (BLOCK + GAP)
            img = np.zeros((n, BLOCKS, BLOCK + GAP), np.uint8)
            img[:, :, :BLOCK] = blocks
            wbase = np.arange(n, dtype=np.int64) * w
            so = (wbase[:, None] + np.arange(BLOCKS, dtype=np.int64)[None, :] * (BLOCK + GAP)).reshape(-1)
            out, cons = streams.compressAt(ids, img.reshape(-1), so, sl, first, np.zeros(n, np.int64), np.zeros(n, np.int32), wbase, np.full(n, w, np.int64), dst,
                                           slots(0), dc)
            assert int(cons.sum()) == n * stride
            b_out[:, :] = out.reshape(n, BLOCKS)
        else:
            img = np.zeros((n, 2, BLOCK), np.uint8)
            wbase = np.arange(n, dtype=np.int64) * (2 * BLOCK)
            for k in range(BLOCKS):
                img[:, k & 1, :] = blocks[:, k, :]      # the producer writes the next block into the other buffer
                he = wbase + ((k - 1) & 1) * BLOCK + BLOCK
                out, cons = streams.compressAt(ids, img.reshape(-1), wbase + (k & 1) * BLOCK, sl, first, he if k else np.zeros(n, np.int64),
                                               np.full(n, BLOCK if k else 0, np.int32), wbase, np.full(n, 2 * BLOCK, np.int64), dst, slots(k), dc)
                assert int(cons.sum()) == n * BLOCK
                b_out[:, k] = out
    # a sample of ext b against the reference on the same places
    L = C.CDLL(O.ref().path)
    L.LZ4_createStream.restype = C.c_void_p
    L.LZ4_freeStream.argtypes = [C.c_void_p]
    L.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    for c in range(0, n, max(1, n // 32)):
        buf = C.create_string_buffer(BLOCKS * (BLOCK + GAP))
        st = L.LZ4_createStream()
        for k in range(BLOCKS):
            at = C.addressof(buf) + (k * (BLOCK + GAP) if calls == 1 else (k & 1) * BLOCK)
            C.memmove(at, raws[c % pool][k * BLOCK:(k + 1) * BLOCK], BLOCK)
            one_dst = C.create_string_buffer(cap)
            r = L.LZ4_compress_fast_continue(st, at, one_dst, BLOCK, cap, 1)
            o = (c * BLOCKS + k) * cap
            assert r == int(b_out[c, k]) and dst[o:o + r].tobytes() == one_dst.raw[:r], "ext b differs from the reference"
        L.LZ4_freeStream(st)
    print("cell ok %d %d" % (int(a_out.astype(np.int64).sum()), int(b_out.astype(np.int64).sum())), flush=True)


def trace_rows(d):
    """[(start ns, duration ns, kernel name)] of the kernel trace rocprofv3 left under d, in order of start"""
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(p) as fh:
            for row in csv.DictReader(fh):
                col = lambda *w: next(v for k, v in row.items() if all(x in k.lower() for x in w))
                rows.append((int(col("start")), int(col("end")) - int(col("start")), col("kernel", "name")))
    return sorted(rows)


def cpu_cell(kind, n, work):
    """the reference on 16 host threads -> (seconds, compressed bytes), or None"""
    from oracle import oracle as O
    exe = os.path.join(work, "cxstream_refbench")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-o", exe, os.path.join(ROOT, "tools", "cxstream_refbench.c"), "-ldl", "-lpthread"])
    pool = os.path.join(work, "pool_%s.bin" % kind)
    with open(pool, "wb") as fh:
        fh.write(b"".join(pool_streams(kind, min(512, n))))
    out = subprocess.check_output([exe, O.ref().path, pool, str(n), "16"], timeout=600).decode().split()
    os.remove(pool)
    return float(out[0]), int(out[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="65536,4096")
    ap.add_argument("--data", default="appf,book1")
    ap.add_argument("--calls", default="1,16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--work", default=None, help="directory for the profiler's output of every cell (default: beside --out, else the current directory)")
    ap.add_argument("--cell-timeout", type=int, default=420)
    ap.add_argument("--worker", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], int(args.worker[1]), int(args.worker[2]))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# cxstream_sweep: kernel time of compress_fast_xstream_cu_kernel (N streams x 16 blocks of 4 KiB, in ONE call and in 16 calls of one block) on")
    emit("# blocks back to back (ext a) beside compress_fast_stream_cu_kernel on the same input (stream), and with one block of history (ext b: two")
    emit("# alternating buffers; in one call every block in a place of its own); rocprofv3 --kernel-trace --stats, one run per cell; cpu = the")
    emit("# reference's LZ4_compress_fast_continue on two alternating buffers, 16 host threads, wall time")
    emit("%6s %8s %6s %11s %11s %11s %9s %9s %10s %10s %8s %9s %9s" % ("data", "streams", "calls", "stream ms", "ext a ms", "ext b ms", "a/stream", "b/a",
                                                                        "a bytes", "b bytes", "b/a size", "cpu ms", "cpu GB/s"))
    work = args.work or (os.path.dirname(os.path.abspath(args.out)) if args.out else os.getcwd())
    os.makedirs(work, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="cxstream_sweep_", dir=work)
    stop = False
    for kind in args.data.split(","):
        for n in (int(v) for v in args.streams.split(",")):
            cpu = cpu_cell(kind, n, tmp)
            for calls in (int(v) for v in args.calls.split(",")):
                d = os.path.join(tmp, "%s_%d_%d" % (kind, n, calls))
                # (timeout -k: the profiler AND the worker behind it end with the time limit; start_new_session + killpg below: nothing of
                # the cell outlives it, whatever ended it)
                cmd = ["timeout", "-k", "10", str(args.cell_timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
                       sys.executable, os.path.abspath(__file__), "--worker", kind, str(n), str(calls)]
                p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
                try:
                    so, se = p.communicate(timeout=args.cell_timeout + 30)
                    status, tail = p.returncode, (se or so)[-300:].replace("\n", " | ")
                    good = status == 0 and "cell ok" in so
                except subprocess.TimeoutExpired:
                    so, status, tail, good = "", 124, "time limit", False
                finally:
                    try:
                        os.killpg(p.pid, signal.SIGKILL)   # (the group is gone after a clean end: nothing to do then)
                    except (ProcessLookupError, PermissionError):
                        pass
                    if p.poll() is None:
                        p.wait()
                if not good:   # (whatever ended it: nothing more is started on the device after a run that failed)
                    emit("# %s %d x %d: the cell's run failed (status %d): %s" % (kind, n, calls, status, tail))
                    emit("# stopping here")
                    stop = True
                    break
                rows = trace_rows(d)
                marker = [t for t, _, name in rows if "compress_fast_chain_cu_kernel" in name]
                s_ns = sum(ns for _, ns, name in rows if "compress_fast_stream_cu_kernel" in name)
                x = [(t, ns) for t, ns, name in rows if "compress_fast_xstream_cu_kernel" in name]
                if not marker or not s_ns or not x:
                    emit("# %s %d x %d: no usable kernel rows (%d rows)" % (kind, n, calls, len(rows)))
                    continue
                a_ns = sum(ns for t, ns in x if t < marker[0])
                b_ns = sum(ns for t, ns in x if t > marker[0])
                a_bytes, b_bytes = (int(v) for v in so.split("cell ok")[1].split()[:2])
                total = float(n) * BLOCK * BLOCKS
                emit("%6s %8d %6d %11.3f %11.3f %11.3f %9.3f %9.3f %10d %10d %8.3f %9.1f %9.2f"
                     % (kind, n, calls, s_ns / 1e6, a_ns / 1e6, b_ns / 1e6, a_ns / s_ns, b_ns / a_ns, a_bytes, b_bytes, b_bytes / a_bytes, cpu[0] * 1e3,
                        total / cpu[0] / 1e9))
                shutil.rmtree(d, ignore_errors=True)
            if stop:
                break
        if stop:
            break
    emit("# ms = total kernel time of the cell's launches (the host path cuts a call into chunks, each a launch); a/stream = the new walk's overhead on")
    emit("# the same input; b/a = one block of history beside the full history, kernel time and (b/a size) output size; cpu ms / GB/s: source bytes over")
    emit("# the reference's wall time on 16 threads.  `stream` is THIS build's stream kernel, instruction-identical to the parent commit's (profiles/xstream_kernel_diff.txt).  %s"
         % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
