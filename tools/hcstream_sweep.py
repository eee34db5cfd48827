#!/usr/bin/env python3
"""tools/hcstream_sweep.py -- what the HC stream compressor for sources that land anywhere costs (lz4hip_compress_hc_stream_batch,
hc_build_stream_kernel + hc_parse_stream_kernel) beside the HC chain compressor (hc_build_chain_kernel + hc_parse_chain_kernel, which
are instruction-identical to the parent commit's: profiles/hcstream_kernel_diff.txt) on one MI355X, and what a history of one block
costs in output size.

The entry points take host pointers, so wall time is staging; what is compared is KERNEL time.  Every cell runs in a child process of
its own under `rocprofv3 --kernel-trace --stats` (nothing else is collected in that run).  A cell is N streams of 16 x 4 KiB blocks at
one HC level, through
  chain     lz4hip_compress_hc_chain_batch, the blocks back to back, ONE call
  stream a  lz4hip_compress_hc_stream_batch on the same blocks back to back, ONE call: no stream ever jumps, so a / chain is what the
            run-end cursor and the two bounds cost
  stream b  lz4hip_compress_hc_stream_batch on the producer's two alternating buffers of 4096 bytes, 16 calls of one block (a call is a
            snapshot, and the next block lands on what this one reads as its dictionary): every block but the first jumps
on Calgary book1 (tests/golden/calgary/book1.xz) and the App. F synthetic blocks (oracle.gen_block); a pool of 512 distinct streams is
tiled to the cell's stream count.  The child checks stream a's sizes against the chain's and a sample of stream b's bytes against the
reference library's ONE LZ4_streamHC_t on the same two buffers.

  python tools/hcstream_sweep.py [--streams 4096,65536] [--data appf,book1] [--level 9] [--out profiles/hcstream_sweep.txt]
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


def worker(kind, n, level):
    """one cell, no timing of its own: chain, stream a, a marker launch, stream b; prints `cell ok <chain bytes> <a bytes> <b bytes>`"""
    import numpy as np
    amd = importlib.import_module("lz4-java_amd")
    from oracle import oracle as O
    B = amd.LZ4HIPBatch
    stride = BLOCK * BLOCKS
    pool = min(512, n)
    raws = pool_streams(kind, pool)
    one = np.frombuffer(b"".join(raws), dtype=np.uint8)
    src = np.tile(one, (n + pool - 1) // pool)[:n * stride]
    blocks = src.reshape(n, BLOCKS, BLOCK)
    cap = BLOCK + BLOCK // 255 + 16
    base = np.arange(n, dtype=np.int64) * stride
    dst = np.zeros(n * BLOCKS * cap, np.uint8)
    all_slots = np.arange(n * BLOCKS, dtype=np.int64) * cap
    # chain: the parent's kernels, one call
    c_out = B.compressHCChain(src, base, np.full(n * BLOCKS, BLOCK, np.int32), np.arange(n + 1, dtype=np.uint32) * np.uint32(BLOCKS), dst, all_slots,
                              np.full(n * BLOCKS, cap, np.int32), None, level)
    # stream a: the same blocks, the same places, fresh streams, one call
    so = (base[:, None] + np.arange(BLOCKS, dtype=np.int64)[None, :] * BLOCK).reshape(-1)
    a_out, _ = B.compressHCStream([(0, 0, 0, 0, 0)] * n, src, so, np.full(n * BLOCKS, BLOCK, np.int32), np.arange(n + 1, dtype=np.uint32) * np.uint32(BLOCKS),
                                  dst, all_slots, np.full(n * BLOCKS, cap, np.int32), level)
    assert (np.asarray(a_out) == np.asarray(c_out)).all(), "stream a's sizes differ from the chain call's"
    # a marker between the two halves of the new kernels' launches: one tiny chain through the fast chain kernel
    B.compressFastChain(bytes(64), [0], [64], [0, 1], bytearray(128), [0], [128])
    # stream b: two alternating buffers, a call per block
    b_out = np.zeros((n, BLOCKS), np.int32)
    img = np.zeros((n, 2, BLOCK), np.uint8)
    wbase = np.arange(n, dtype=np.int64) * (2 * BLOCK)
    state = [(0, 0, 0, 0, 0)] * n
    first = np.arange(n + 1, dtype=np.uint32)
    sl, dc = np.full(n, BLOCK, np.int32), np.full(n, cap, np.int32)
    for k in range(BLOCKS):
        img[:, k & 1, :] = blocks[:, k, :]      # the producer writes the next block into the other buffer
        out, state = B.compressHCStream(state, img.reshape(-1), wbase + (k & 1) * BLOCK, sl, first, dst, np.ascontiguousarray(all_slots[k::BLOCKS]), dc, level)
        b_out[:, k] = out
    # a sample of stream b against the reference on the same two buffers
    L = C.CDLL(O.ref().path)
    L.LZ4_createStreamHC.restype = C.c_void_p
    L.LZ4_freeStreamHC.argtypes = [C.c_void_p]
    L.LZ4_resetStreamHC_fast.argtypes = [C.c_void_p, C.c_int]
    L.LZ4_compress_HC_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    for c in range(0, n, max(1, n // 32)):
        buf = C.create_string_buffer(2 * BLOCK)
        st = L.LZ4_createStreamHC()
        L.LZ4_resetStreamHC_fast(st, level)
        for k in range(BLOCKS):
            at = C.addressof(buf) + (k & 1) * BLOCK
            C.memmove(at, raws[c % pool][k * BLOCK:(k + 1) * BLOCK], BLOCK)
            one_dst = C.create_string_buffer(cap)
            r = L.LZ4_compress_HC_continue(st, at, one_dst, BLOCK, cap)
            o = (c * BLOCKS + k) * cap
            assert r == int(b_out[c, k]) and dst[o:o + r].tobytes() == one_dst.raw[:r], "stream b differs from the reference"
        L.LZ4_freeStreamHC(st)
    print("cell ok %d %d %d" % (int(np.asarray(c_out, dtype=np.int64).sum()), int(np.asarray(a_out, dtype=np.int64).sum()), int(b_out.astype(np.int64).sum())),
          flush=True)


def trace_rows(d):
    """[(start ns, duration ns, kernel name)] of the kernel trace rocprofv3 left under d, in order of start"""
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(p) as fh:
            for row in csv.DictReader(fh):
                col = lambda *w: next(v for k, v in row.items() if all(x in k.lower() for x in w))
                rows.append((int(col("start")), int(col("end")) - int(col("start")), col("kernel", "name")))
    return sorted(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="4096,65536")
    ap.add_argument("--data", default="appf,book1")
    ap.add_argument("--level", type=int, default=9)
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

    emit("# hcstream_sweep: kernel time of hc_build_stream_kernel + hc_parse_stream_kernel (N streams x 16 blocks of 4 KiB, level %d) on blocks back to" % args.level)
    emit("# back in ONE call (a) beside hc_build_chain_kernel + hc_parse_chain_kernel on the same input (chain), and on two alternating buffers in 16")
    emit("# calls of one block (b); rocprofv3 --kernel-trace --stats, one run per cell")
    emit("%6s %8s %10s %10s %10s %10s %10s %10s %8s %8s %8s %8s %11s %11s %8s" % ("data", "streams", "chain bld", "chain prs", "a build", "a parse", "b build", "b parse",
                                                                             "a/chain", "bld a/c", "prs a/c", "b/a", "a bytes", "b bytes", "b/a size"))
    work = args.work or (os.path.dirname(os.path.abspath(args.out)) if args.out else os.getcwd())
    os.makedirs(work, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="hcstream_sweep_", dir=work)
    stop = False
    for kind in args.data.split(","):
        for n in (int(v) for v in args.streams.split(",")):
            d = os.path.join(tmp, "%s_%d" % (kind, n))
            # (timeout -k: the profiler AND the worker behind it end with the time limit; start_new_session + killpg below: nothing of the
            # cell outlives it, whatever ended it)
            cmd = ["timeout", "-k", "10", str(args.cell_timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--worker", kind, str(n), str(args.level)]
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
                emit("# %s %d: the cell's run failed (status %d): %s" % (kind, n, status, tail))
                emit("# stopping here")
                stop = True
                break
            rows = trace_rows(d)
            marker = [t for t, _, name in rows if "compress_fast_chain_cu_kernel" in name]
            total = lambda word, lo, hi: sum(ns for t, ns, name in rows if word in name and lo < t < hi)
            if not marker:
                emit("# %s %d: no usable kernel rows (%d rows)" % (kind, n, len(rows)))
                continue
            m, inf = marker[0], float("inf")
            cb, cp = total("hc_build_chain_kernel", -1, inf), total("hc_parse_chain_kernel", -1, inf)
            ab, apn = total("hc_build_stream_kernel", -1, m), total("hc_parse_stream_kernel", -1, m)
            bb, bp = total("hc_build_stream_kernel", m, inf), total("hc_parse_stream_kernel", m, inf)
            if not (cb and cp and ab and apn and bb and bp):
                emit("# %s %d: no usable kernel rows (%d rows)" % (kind, n, len(rows)))
                continue
            c_bytes, a_bytes, b_bytes = (int(v) for v in so.split("cell ok")[1].split()[:3])
            emit("%6s %8d %10.3f %10.3f %10.3f %10.3f %10.3f %10.3f %8.3f %8.3f %8.3f %8.3f %11d %11d %8.3f"
                 % (kind, n, cb / 1e6, cp / 1e6, ab / 1e6, apn / 1e6, bb / 1e6, bp / 1e6, (ab + apn) / (cb + cp), ab / cb, apn / cp, (bb + bp) / (ab + apn),
                    a_bytes, b_bytes, b_bytes / a_bytes))
            shutil.rmtree(d, ignore_errors=True)
        if stop:
            break
    emit("# ms = total kernel time of the cell's launches (the host path cuts a call into chunks, each a launch); a/chain = the new pair beside the chain")
    emit("# pair on the same input (bld / prs a/c: the build and the parse kernels apart); b/a = one block of history beside the full history, kernel time")
    emit("# and (b/a size) output size.  `chain` is THIS build's chain kernels, instruction-identical to the parent commit's.  %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
