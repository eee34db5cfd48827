#!/usr/bin/env python3
"""usage: tools/container_many_sweep.py [--out FILE] [--max-gib G] [--loop-items K]      (needs a GPU: there is no CPU fallback)
       tools/container_many_sweep.py --trace-child                                       (the program rocprofv3 wraps, see below)

Wall time of reading N small containers: ONE lz4hip_container_decode_many against a loop of N lz4hip_container_decode calls in the
same build (the loop is the parent's code: profiles/container_many_kernel_diff.txt shows every kernel it runs unchanged).

  items   N = 256, 4096, 65536, each one block of 4 KiB or four blocks of 64 KiB
  data    SURVEY.md App. F synthetic blocks (oracle.gen_block) and book1 (tests/golden/calgary), compressed with the reference library
  kinds   LZ4 Frame bodies (block checksums on) and LZ4Block streams

Every time is a host clock around a call that returns after its last device synchronise.  Both sides are warmed up with the shape
they are timed on; the many-call is the best and the median of 5 calls; the loop is timed over at most --loop-items items (default
1024: a loop's time per item does not depend on how long the loop is, which the N = 256 and N = 4096 rows show) and reported per
item.  The two are timed alternately in the same process.  Both results are compared item by item before anything is timed.  A
shape whose decoded bytes exceed --max-gib (default 4) of destination is skipped and says so: frames ask for max_block per
compressed block, so 65536 items of four 64 KiB blocks are 16 GiB.

Kernel time comes from a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -o many -- python tools/container_many_sweep.py --trace-child
runs one many-call of 4096 frames of one 4 KiB block after a warm-up call; the kernels' names are stable (container_walk_many_kernel,
container_verdict_many_kernel, the decoders', xxh_multi_kernel, container_raw_kernel, pack_copy_kernel)."""
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
import container_many_common as cm   # noqa: E402 -- the tests' builders of bodies and of the call's arrays
from conftest import calgary         # noqa: E402
from oracle import oracle as O       # noqa: E402


def make_items(ref, kind, data, n, sizes):
    """n items; item i holds the blocks data[o_i ..] cut into `sizes` (a few hundred distinct bodies, repeated)"""
    distinct, span = [], sum(sizes)
    for k in range(min(n, 256)):
        o = (k * 7919) % max(1, len(data) - span)
        blocks = cm.cut(data[o:o + span], sizes)
        distinct.append(cm.frame_body(ref, blocks, True) if kind == 0 else cm.block_stream(ref, blocks, 65536))
    return [("i", kind, distinct[i % len(distinct)], 65536, kind == 0) for i in range(n)]


def timed(f):
    t = time.perf_counter()
    f()
    return time.perf_counter() - t


def many_call(L, kind, pk, n_max, bufs):
    dst, sizes, info, doff, first, cap, scap = bufs
    rc = L.lz4hip_container_decode_many(*pk.head(kind, n_max), cm._p(dst, C.c_uint8), cap, cm._p(doff, C.c_uint64), cm._p(first, C.c_uint32),
                                        cm._p(sizes, C.c_int32), scap, cm._p(info, C.c_uint64))
    assert rc == 0, L.lz4hip_last_error()


def loop_calls(L, kind, items, n_max, k):
    dst, sizes, info = np.empty(n_max * 65536, np.uint8), np.zeros(n_max, np.int32), np.zeros(5, np.uint64)
    bodies = [np.frombuffer(it[2], dtype=np.uint8) for it in items[:k]]
    def run():
        for it, b in zip(items, bodies):
            rc = L.lz4hip_container_decode(kind, 1 if it[4] else 0, b.ctypes.data, len(b), it[3], n_max, dst.ctypes.data, len(dst), cm._p(sizes, C.c_int32),
                                           cm._p(info, C.c_uint64))
            assert rc == 0, L.lz4hip_last_error()
    return run


def sweep(args):
    amd = importlib.import_module("lz4-java_amd")
    L, ref = amd.lib(), O.ref()
    book1 = calgary("book1")
    appf = b"".join(O.gen_block(65536, i) for i in range(12))
    lines = ["container_many_sweep: one lz4hip_container_decode_many against a loop of lz4hip_container_decode calls, same build, wall time",
             "%-8s %-6s %-10s %6s | %12s %12s | %12s | %10s %10s | %7s" % ("kind", "data", "item", "N", "many ms best", "many ms med", "loop us/item",
                                                                            "many us/it", "MB/s many", "ratio")]
    n_max = 8
    for kind, kname in ((0, "frame"), (1, "lz4block")):
        for dname, data in (("appF", appf), ("book1", book1)):
            for sname, sizes in (("1x4KiB", [4096]), ("4x64KiB", [65536] * 4)):
                for n in (256, 4096, 65536):
                    decoded = n * sum(sizes)
                    if decoded > args.max_gib * (1 << 30):
                        lines.append("%-8s %-6s %-10s %6d | skipped: %.1f GiB of decoded bytes in one call exceed --max-gib" % (kname, dname, sname, n, decoded / 2 ** 30))
                        continue
                    items = make_items(ref, kind, data, n, sizes)
                    pk = cm.Packed(items)
                    nb, need = cm.bound_many(L, kind, pk, n_max)
                    cap, scap = int(need.sum()), int(nb.sum())
                    bufs = (np.empty(cap + 1, np.uint8), np.zeros(scap + 1, np.int32), np.zeros(5 * n, np.uint64), np.zeros(n + 1, np.uint64),
                            np.zeros(n + 1, np.uint32), cap, scap)
                    k = min(n, args.loop_items)
                    loop = loop_calls(L, kind, items, n_max, k)
                    many_call(L, kind, pk, n_max, bufs)          # warm-up, and the comparison of the two before anything is timed
                    loop()
                    got = cm.decode_many(L, kind, items[:64], n_max)
                    for it, g in zip(items[:64], got):
                        assert tuple(amd.LZ4HIPBatch.containerDecode(kind, it[2], it[3], n_max, it[4])) == g and len(g[0]) == sum(sizes)
                    assert int(bufs[3][n]) == decoded
                    tm, tl = [], []
                    for _ in range(5):                           # alternating
                        tm.append(timed(lambda: many_call(L, kind, pk, n_max, bufs)))
                        tl.append(timed(loop))
                    best, med, lp = min(tm), statistics.median(tm), statistics.median(tl) / k
                    lines.append("%-8s %-6s %-10s %6d | %12.3f %12.3f | %12.1f | %10.2f %10.0f | %7.1f" %
                                 (kname, dname, sname, n, best * 1e3, med * 1e3, lp * 1e6, med / n * 1e6, decoded / med / 1e6, lp / (med / n)))
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


def trace_child():
    amd = importlib.import_module("lz4-java_amd")
    L, ref = amd.lib(), O.ref()
    items = make_items(ref, 0, calgary("book1"), 4096, [4096])
    pk = cm.Packed(items)
    nb, need = cm.bound_many(L, 0, pk, 8)
    cap, scap = int(need.sum()), int(nb.sum())
    bufs = (np.empty(cap + 1, np.uint8), np.zeros(scap + 1, np.int32), np.zeros(5 * 4096, np.uint64), np.zeros(4097, np.uint64), np.zeros(4097, np.uint32), cap, scap)
    for _ in range(2):
        many_call(L, 0, pk, 8, bufs)
    assert int(bufs[3][4096]) == 4096 * 4096


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--max-gib", type=float, default=4.0)
    ap.add_argument("--loop-items", type=int, default=1024)
    ap.add_argument("--trace-child", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        trace_child()
    else:
        sweep(a)
