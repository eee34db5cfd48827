#!/usr/bin/env python3
"""tools/caccel_sweep.py -- what LZ4_compress_fast_continue's acceleration buys the linked-block compressors on one MI355X:
kernel time of compress_fast_chain_accel_cu_kernel (lz4hip_compress_fast_chain_accel_batch) at acceleration 2, 8 and 64 beside this
build's compress_fast_chain_cu_kernel (acceleration 1) on the same data, and the same for the resident-stream kernels
(compress_fast_stream_accel_cu_kernel beside compress_fast_stream_cu_kernel) in 16 calls of one block.

The entry points take host pointers, so wall time is staging; what is compared is KERNEL time.  Every cell runs in a child process of
its own under `rocprofv3 --kernel-trace --stats` (nothing else is collected in that run), and the kernels' total times are read from
the child's kernel-stats table.  A cell is N chains (or streams) of 16 x 4 KiB blocks of Calgary book1 (tests/golden/calgary/book1.xz)
or of the App. F synthetic blocks (oracle.gen_block); a pool of 512 distinct chains is tiled to the cell's count.  The child runs the
acceleration-1 call and the accelerated call on the same source and prints both compressed sizes: `size` is the accelerated output
relative to acceleration 1.  Mode `cpu`: the reference library's LZ4_compress_fast_continue on the same chains, ONE LZ4_stream_t each, on 16
host threads (tools/caccel_refbench.c, built into the work directory), wall time, at acceleration 1 and at the cell's.

  python tools/caccel_sweep.py [--chains 65536,4096] [--data appf,book1] [--accel 2,8,64] [--modes chain,stream,cpu] [--out profiles/caccel_sweep.txt]
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
KERNELS = {"chain": ("compress_fast_chain_cu_kernel", "compress_fast_chain_accel_cu_kernel"),
           "stream": ("compress_fast_stream_cu_kernel", "compress_fast_stream_accel_cu_kernel")}


def worker(mode, kind, n, accel):
    """one cell, no timing of its own: the call(s) at acceleration 1, then at `accel`; prints `cell ok <bytes at 1> <bytes at accel>`"""
    import numpy as np
    amd = importlib.import_module("lz4-java_amd")
    book = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "calgary", "book1.xz"), "rb").read())
    stride = BLOCK * BLOCKS
    pool = min(512, n)
    one = np.frombuffer(b"".join(pool_chain(kind, k, book) for k in range(pool)), dtype=np.uint8)
    src = np.tile(one, (n + pool - 1) // pool)[:n * stride]
    cap = BLOCK + BLOCK // 255 + 16
    base = np.arange(n, dtype=np.int64) * stride
    dst = np.zeros(n * BLOCKS * cap, np.uint8)
    sizes = []
    for a in (1, accel):
        if mode == "chain":
            out, cons = amd.LZ4HIPBatch.compressFastChain(src, base, np.full(n * BLOCKS, BLOCK, np.int32), np.arange(n + 1, dtype=np.uint32) * np.uint32(BLOCKS),
                                                          dst, np.arange(n * BLOCKS, dtype=np.int64) * cap, np.full(n * BLOCKS, cap, np.int32), acceleration=a)
            assert int(cons.sum()) == n * stride, "a chain of the cell stopped"
            sizes.append(int(out.astype(np.int64).sum()))
        else:
            total = 0
            ids = np.arange(n, dtype=np.uint32)
            with amd.CompressStreams(n) as streams:
                for k in range(BLOCKS):
                    out, cons = streams.compress(ids, src, base + k * BLOCK, np.full(n, BLOCK, np.int32), np.arange(n + 1, dtype=np.uint32), dst,
                                                 (np.arange(n, dtype=np.int64) * BLOCKS + k) * cap, np.full(n, cap, np.int32), np.full(n, k * BLOCK, np.int32),
                                                 acceleration=a)
                    assert int(cons.sum()) == n * BLOCK, "a stream of the cell stopped"
                    total += int(out.astype(np.int64).sum())
            sizes.append(total)
    print("cell ok %d %d" % tuple(sizes), flush=True)


def pool_chain(kind, k, book):
    """chain k of the pool: 16 x 4 KiB of book1 or of the App. F generator"""
    from oracle import oracle as O
    stride = BLOCK * BLOCKS
    if kind == "book1":
        o = (k * 104729) % (len(book) - stride)
        return book[o:o + stride]
    return O.gen_block(stride, 1000 + k)


def cpu_cells(kind, n, accels, work):
    """the reference on 16 host threads at acceleration 1 and at each of `accels` -> {acceleration: (seconds, compressed bytes)}"""
    from oracle import oracle as O
    exe = os.path.join(work, "caccel_refbench")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-o", exe, os.path.join(ROOT, "tools", "caccel_refbench.c"), "-ldl", "-lpthread"])
    book = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "calgary", "book1.xz"), "rb").read())
    pool = os.path.join(work, "pool_%s.bin" % kind)
    with open(pool, "wb") as fh:
        fh.write(b"".join(pool_chain(kind, k, book) for k in range(min(512, n))))
    res = {}
    for a in (1,) + tuple(accels):
        out = subprocess.check_output([exe, O.ref().path, pool, str(n), "16", str(a)], timeout=600).decode().split()
        res[a] = (float(out[0]), int(out[2]))
    os.remove(pool)
    return res


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
    ap.add_argument("--chains", default="65536,4096")
    ap.add_argument("--data", default="appf,book1")
    ap.add_argument("--accel", default="2,8,64")
    ap.add_argument("--modes", default="chain,stream")
    ap.add_argument("--out", default=None)
    ap.add_argument("--work", default=None, help="directory for the profiler's output of every cell (default: beside --out, else the current directory)")
    ap.add_argument("--cell-timeout", type=int, default=300)
    ap.add_argument("--worker", nargs=4, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1], int(args.worker[2]), int(args.worker[3]))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# caccel_sweep: kernel time of the accelerated linked-block kernels beside this build's acceleration-1 kernels on the same data")
    emit("# (N chains of 16 x 4 KiB blocks in one call; N streams in 16 calls of one block); rocprofv3 --kernel-trace --stats, one run per cell")
    emit("%6s %6s %8s %6s %12s %12s %12s %12s %8s %8s" % ("mode", "data", "chains", "accel", "accel-1 ms", "accel ms", "accel-1 GB/s", "accel GB/s", "speed", "size"))
    work = args.work or (os.path.dirname(os.path.abspath(args.out)) if args.out else os.getcwd())
    os.makedirs(work, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="caccel_sweep_", dir=work)
    cells = [(m, kind, n, a) for m in args.modes.split(",") if m != "cpu" for kind in args.data.split(",") for n in (int(v) for v in args.chains.split(","))
             for a in (int(v) for v in args.accel.split(","))]
    for mode, kind, n, accel in cells:
        d = os.path.join(tmp, "%s_%s_%d_%d" % (mode, kind, n, accel))
        # (timeout -k: the profiler AND the worker behind it end with the time limit; start_new_session + killpg below: nothing of the
        # cell outlives it, whatever ended it)
        cmd = ["timeout", "-k", "10", str(args.cell_timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--worker", mode, kind, str(n), str(accel)]
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
            emit("# %s %s %d at %d: the cell's run failed (status %d): %s" % (mode, kind, n, accel, status, tail))
            emit("# stopping here")
            break
        ks = kernel_ns(d)
        plain_name, accel_name = KERNELS[mode]
        plain = [v for k, v in ks.items() if plain_name in k]
        fast = [v for k, v in ks.items() if accel_name in k]
        if not plain or not fast:
            emit("# %s %s %d at %d: no kernel-stats rows for the two kernels (%d rows)" % (mode, kind, n, accel, len(ks)))
            continue
        size1, size_a = (int(v) for v in so.split("cell ok")[1].split()[:2])
        p_ns, a_ns = plain[0][1], fast[0][1]
        total = float(n) * BLOCK * BLOCKS
        emit("%6s %6s %8d %6d %12.3f %12.3f %12.2f %12.2f %8.2f %8.3f" % (mode, kind, n, accel, p_ns / 1e6, a_ns / 1e6, total / p_ns, total / a_ns, p_ns / a_ns, size_a / size1))
        shutil.rmtree(d, ignore_errors=True)
    if "cpu" in args.modes.split(","):
        accels = tuple(int(v) for v in args.accel.split(","))
        for kind in args.data.split(","):
            for n in (int(v) for v in args.chains.split(",")):
                res = cpu_cells(kind, n, accels, tmp)
                total = float(n) * BLOCK * BLOCKS
                for a in accels:
                    emit("%6s %6s %8d %6d %12.3f %12.3f %12.2f %12.2f %8.2f %8.3f" % ("cpu", kind, n, a, res[1][0] * 1e3, res[a][0] * 1e3, total / res[1][0] / 1e9,
                                                                                     total / res[a][0] / 1e9, res[1][0] / res[a][0], res[a][1] / res[1][1]))
        emit("# cpu = the reference's LZ4_compress_fast_continue on the same chains, ONE LZ4_stream_t each, 16 host threads, wall time (best of three)")
    emit("# ms = total kernel time of the cell's launches (the host path cuts a call into chunks of 64 MiB of source, each a launch); GB/s = source")
    emit("# bytes / kernel time; speed = acceleration-1 kernel time / accelerated kernel time (above 1: faster); size = accelerated output bytes /")
    emit("# acceleration-1 output bytes.  The acceleration-1 kernels are instruction-identical to the parent's (profiles/caccel_kernel_diff.txt).")
    emit("# %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
