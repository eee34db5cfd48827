#!/usr/bin/env python3
"""usage: tools/container_write_many_sweep.py [--out FILE] [--loop-items K]      (needs a GPU: there is no CPU fallback)
       tools/container_write_many_sweep.py --trace-child                       (the program rocprofv3 wraps, see below)

Wall time of writing N small containers: ONE lz4hip_container_blocks_many against a loop of N lz4hip_container_blocks calls in the
same build (the loop is the parent's code: profiles/container_write_many_kernel_diff.txt shows every kernel it runs unchanged).

  items   N = 256, 4096, 65536 of one block of 4 KiB; N = 4096 of four blocks of 64 KiB
  data    SURVEY.md App. F synthetic blocks (oracle.gen_block) and book1 (tests/golden/calgary)
  kinds   LZ4 Frame blocks (block checksums on, 15 and 8 bytes of gap for the header, the end mark and the content checksum, content
          hash asked) and LZ4Block blocks (21 bytes of gap behind for the empty end block); level 0

Every time is a host clock around a call that returns after its last device synchronise.  Both sides are warmed up with the shape
they are timed on; the many-call is the best and the median of 5 calls; the loop is timed over at most --loop-items items (default
1024) and reported per item.  The two are timed alternately in the same process.  The first 64 items of both are compared before
anything is timed.

Kernel time comes from a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -o many -- python tools/container_write_many_sweep.py --trace-child
runs one many-call of 4096 frames of one 4 KiB block after a warm-up call; the kernels' names are stable (container_layout_many_kernel,
the compressors', xxh_multi_kernel, container_scan_many_kernel, container_copy_many_kernel, container_put_hashes_many_kernel)."""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import container_write_many_common as wm   # noqa: E402 -- the tests' builders of the call's arrays
from conftest import calgary               # noqa: E402
from oracle import oracle as O             # noqa: E402


def make_items(kind, data, n, size, bs):
    """n items of `size` bytes cut into bs pieces (a few hundred distinct payloads, repeated)"""
    distinct = [data[(k * 7919) % max(1, len(data) - size):][:size] for k in range(min(n, 256))]
    return [("i", distinct[i % len(distinct)], bs, kind == 0, 15 if kind == 0 else 0, 8 if kind == 0 else 21, kind == 0) for i in range(n)]


def timed(f):
    t = time.perf_counter()
    f()
    return time.perf_counter() - t


def many_call(L, kind, pk, bufs):
    dst, doff, hashes, cap = bufs
    rc = L.lz4hip_container_blocks_many(*pk.head(kind, 0), wm._p(dst, C.c_uint8), cap, wm._p(doff, C.c_uint64), wm._p(hashes, C.c_uint32))
    assert rc == 0, L.lz4hip_last_error()


def loop_calls(L, kind, items, k):
    size, bs = len(items[0][1]), items[0][2]
    cap = size + (size + bs - 1) // bs * 21
    dst, out = np.empty(cap, np.uint8), C.c_uint64(0)
    srcs = [np.frombuffer(it[1], dtype=np.uint8) for it in items[:k]]

    def run():
        for s in srcs:
            rc = L.lz4hip_container_blocks(kind, 1 if kind == 0 else 0, 0, s.ctypes.data, len(s), bs, dst.ctypes.data, cap, C.byref(out))
            assert rc == 0, L.lz4hip_last_error()
    return run


def buffers(L, kind, pk):
    nb, need = wm.bound_many(L, kind, pk)
    cap = int(need.sum())
    return (np.empty(cap + 1, np.uint8), np.zeros(pk.n + 1, np.uint64), np.zeros(pk.n + 1, np.uint32), cap)


def sweep(args):
    amd = importlib.import_module("lz4-java_amd")
    L = amd.lib()
    book1 = calgary("book1")
    appf = b"".join(O.gen_block(65536, i) for i in range(12))
    lines = ["container_write_many_sweep: one lz4hip_container_blocks_many against a loop of lz4hip_container_blocks calls, same build, wall time",
             "%-8s %-6s %-10s %6s | %12s %12s | %12s | %10s %10s | %7s" % ("kind", "data", "item", "N", "many ms best", "many ms med", "loop us/item",
                                                                            "many us/it", "MB/s many", "ratio")]
    for kind, kname in ((0, "frame"), (1, "lz4block")):
        for dname, data in (("appF", appf), ("book1", book1)):
            for sname, size, bs, ns in (("1x4KiB", 4096, 4096, (256, 4096, 65536)), ("4x64KiB", 4 * 65536, 65536, (4096,))):
                for n in ns:
                    items = make_items(kind, data, n, size, bs)
                    pk = wm.Packed(items)
                    bufs = buffers(L, kind, pk)
                    k = min(n, args.loop_items)
                    loop = loop_calls(L, kind, items, k)
                    many_call(L, kind, pk, bufs)                 # warm-up, and the comparison of the two before anything is timed
                    loop()
                    for it, (blocks, h) in zip(items[:64], wm.write_many(L, kind, 0, items[:64])):
                        assert blocks == amd.LZ4HIPBatch.containerBlocks(kind, it[1], it[2], it[3], 0)
                    tm, tl = [], []
                    for _ in range(5):                           # alternating
                        tm.append(timed(lambda: many_call(L, kind, pk, bufs)))
                        tl.append(timed(loop))
                    best, med, lp = min(tm), statistics.median(tm), statistics.median(tl) / k
                    lines.append("%-8s %-6s %-10s %6d | %12.3f %12.3f | %12.1f | %10.2f %10.0f | %7.1f" %
                                 (kname, dname, sname, n, best * 1e3, med * 1e3, lp * 1e6, med / n * 1e6, n * size / med / 1e6, lp / (med / n)))
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


def trace_child():
    amd = importlib.import_module("lz4-java_amd")
    L = amd.lib()
    items = make_items(0, calgary("book1"), 4096, 4096, 4096)
    pk = wm.Packed(items)
    bufs = buffers(L, 0, pk)
    for _ in range(2):
        many_call(L, 0, pk, bufs)
    assert int(bufs[1][4096]) > 4096 * 27


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--loop-items", type=int, default=1024)
    ap.add_argument("--trace-child", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        trace_child()
    else:
        sweep(a)
