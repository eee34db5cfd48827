#!/usr/bin/env python3
"""tools/cstream_sweep.py -- what the state traffic of the resident-stream compressor costs (lz4hip_compress_fast_stream_batch,
compress_fast_stream_cu_kernel) on one MI355X: a stream moves 64 KB of table per call -- 32 KB in, 32 KB out -- whatever its blocks' sizes.

The entry point takes host pointers, so wall time is staging; what is compared is KERNEL time.  Every cell runs in a child process of
its own under `rocprofv3 --kernel-trace --stats` (nothing else is collected in that run), and the kernels' total times are read from
the child's kernel-stats table:
  stream   compress_fast_stream_cu_kernel: N streams x 16 calls x one 4 KiB block, and x 4 calls x four blocks; every stream's data is
           left in place, so call k passes everything the stream has consumed (at most 64 KiB) as its history
  chain    compress_fast_chain_cu_kernel on the same 16 blocks per chain in ONE call (lz4hip_compress_fast_chain_batch): no state traffic
on Calgary book1 (tests/golden/calgary/book1.xz) and the App. F synthetic blocks (oracle.gen_block); a pool of 512 distinct streams is
tiled to the cell's stream count.  The child also checks that the streams' sizes and a sample of their bytes equal the chain call's.

  python tools/cstream_sweep.py [--streams 65536,4096] [--data appf,book1] [--out profiles/cstream_sweep.txt]
"""
import argparse
import csv
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
CUTS = (16, 4)    # calls per stream


def worker(kind, n, calls):
    """one cell, no timing of its own: the stream calls, then the chain call; prints `cell ok <compressed bytes>`"""
    import numpy as np
    amd = importlib.import_module("lz4-java_amd")
    from oracle import oracle as O
    book = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "calgary", "book1.xz"), "rb").read())
    stride = BLOCK * BLOCKS
    pool = min(512, n)
    def raw(k):
        if kind == "book1":
            o = (k * 104729) % (len(book) - stride)
            return book[o:o + stride]
        return O.gen_block(stride, 1000 + k)
    one = np.frombuffer(b"".join(raw(k) for k in range(pool)), dtype=np.uint8)
    src = np.tile(one, (n + pool - 1) // pool)[:n * stride]
    cap = BLOCK + BLOCK // 255 + 16
    per = BLOCKS // calls
    ids = np.arange(n, dtype=np.uint32)
    s_out = np.zeros((n, BLOCKS), np.int32)
    s_dst = np.zeros(n * BLOCKS * cap, np.uint8)
    base = np.arange(n, dtype=np.int64) * stride
    with amd.CompressStreams(n) as streams:
        for k in range(calls):
            done = k * per * BLOCK
            cso = base + done
            pre = np.full(n, done, np.int32)
            sl = np.full(n * per, BLOCK, np.int32)
            first = (np.arange(n + 1, dtype=np.uint32) * np.uint32(per))
            blk = (np.arange(n, dtype=np.int64)[:, None] * BLOCKS + np.arange(k * per, (k + 1) * per, dtype=np.int64)[None, :]).reshape(-1)
            do = blk * cap
            dc = np.full(n * per, cap, np.int32)
            out, cons = streams.compress(ids, src, cso, sl, first, s_dst, do, dc, pre)
            assert int(cons.sum()) == n * per * BLOCK, "a stream of the cell stopped"
            s_out[:, k * per:(k + 1) * per] = out.reshape(n, per)
    sample = {c: s_dst[c * BLOCKS * cap:(c + 1) * BLOCKS * cap].copy() for c in range(0, n, max(1, n // 64))}
    sl = np.full(n * BLOCKS, BLOCK, np.int32)
    do = np.arange(n * BLOCKS, dtype=np.int64) * cap
    # (the chain call writes the same slots again)
    out, cons = amd.LZ4HIPBatch.compressFastChain(src, base, sl, np.arange(n + 1, dtype=np.uint32) * np.uint32(BLOCKS), s_dst, do,
                                                  np.full(n * BLOCKS, cap, np.int32))
    assert int(cons.sum()) == n * stride
    assert (out.reshape(n, BLOCKS) == s_out).all(), "the streams' sizes differ from the one-call chain's"
    for c, was in sample.items():
        for i in range(BLOCKS):
            r = int(s_out[c, i])
            assert (was[i * cap:i * cap + r] == s_dst[(c * BLOCKS + i) * cap:(c * BLOCKS + i) * cap + r]).all(), "the streams' bytes differ from the one-call chain's"
    print("cell ok %d" % int(s_out.astype(np.int64).sum()), flush=True)


def kernel_ns(d):
    """{kernel name: (calls, total ns)} of the kernel-stats table rocprofv3 left under d"""
    res = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(p) as fh:
            for row in csv.DictReader(fh):
                col = lambda *w: next(v for k, v in row.items() if all(x in k.lower() for x in w))
                res[col("name")] = (int(col("calls")), int(float(col("total"))))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="65536,4096")
    ap.add_argument("--data", default="appf,book1")
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

    emit("# cstream_sweep: kernel time of compress_fast_stream_cu_kernel (N streams x CALLS calls x 16/CALLS blocks of 4 KiB) beside")
    emit("# compress_fast_chain_cu_kernel on the same 16 blocks per chain in ONE call; rocprofv3 --kernel-trace --stats, one run per cell")
    emit("%6s %8s %6s %14s %14s %12s %12s %8s %14s" % ("data", "streams", "calls", "stream ms", "chain ms", "stream GB/s", "chain GB/s", "ratio", "state GB/s"))
    work = args.work or (os.path.dirname(os.path.abspath(args.out)) if args.out else os.getcwd())
    os.makedirs(work, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="cstream_sweep_", dir=work)
    for kind in args.data.split(","):
        for n in (int(v) for v in args.streams.split(",")):
            for calls in CUTS:
                d = os.path.join(tmp, "%s_%d_%d" % (kind, n, calls))
                # (timeout -k: the profiler AND the worker behind it end with the time limit; start_new_session + killpg below: nothing of the
                # cell outlives it, whatever ended it)
                cmd = ["timeout", "-k", "10", str(args.cell_timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
                       sys.executable, os.path.abspath(__file__), "--worker", kind, str(n), str(calls)]
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
                    emit("# %s %d x %d: the cell's run failed (status %d): %s" % (kind, n, calls, status, tail))
                    emit("# stopping here")
                    break
                ks = kernel_ns(d)
                st = [v for k, v in ks.items() if "compress_fast_stream_cu_kernel" in k]
                ch = [v for k, v in ks.items() if "compress_fast_chain_cu_kernel" in k]
                if not st or not ch:
                    emit("# %s %d x %d: no kernel-stats rows for the two kernels (%d rows)" % (kind, n, calls, len(ks)))
                    continue
                s_ns, c_ns = st[0][1], ch[0][1]
                total = float(n) * BLOCK * BLOCKS
                emit("%6s %8d %6d %14.3f %14.3f %12.2f %12.2f %8.2f %14.1f"
                     % (kind, n, calls, s_ns / 1e6, c_ns / 1e6, total / s_ns, total / c_ns, s_ns / c_ns, float(n) * calls * 65536 / s_ns))
                shutil.rmtree(d, ignore_errors=True)
            else:
                continue
            break
        else:
            continue
        break
    emit("# stream ms / chain ms = total kernel time of the cell's launches (the host path cuts a call into chunks of 64 MiB of source, each a launch);")
    emit("# GB/s = source bytes / kernel time; ratio = stream / chain kernel time; state GB/s = streams x calls x 64 KB of table moved / stream kernel time")
    emit("# (an upper bound on the traffic: a fresh stream loads no table).  The chain kernel is instruction-identical to the parent's")
    emit("# (profiles/cstream_kernel_diff.txt).  %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
