#!/usr/bin/env python3
"""tools/accel_sweep.py -- throughput and ratio of LZ4_compress_fast(..., acceleration) on one MI355X.

Device-resident workloads (nothing crosses PCIe while timing):
  appf64k   65536 x 64 KiB SURVEY.md App. F blocks (DeviceBatch.gen_blocks: the headline's blocks)
  book64k   8192 x 64 KiB slices of Calgary book1 (tests/golden/calgary/book1.xz, seeded offsets)
  appf4m    1024 x 4 MiB App. F blocks, win 4096 (byU32 tables)
Accelerations 1, 2, 4, 8, 16 and 64.  Acceleration 1 is the library's plain fast compressor (the lean core with writer wavefronts
and the window-parallel core, as lz4hip_compress_fast_batch_dev routes it); every other value runs compress_fast_accel_cu_kernel.

Per cell: one warm-up launch, then --reps timed launches, each between its own pair of HIP events on torch's stream; reported: input
GB/s of the median launch, the spread (min .. max GB/s over the launches), the ratio (input / output bytes), a decode round trip of
the whole batch (safe decompress on the device, compared with the source on the device) and -- where the reference library is on the
box -- the bytes of a seeded sample of blocks against its LZ4_compress_fast.

  python tools/accel_sweep.py [--reps 7] [--out profiles/accel_sweep.txt] [--only appf64k,book64k] [--accels 1,2,8]
Kernel times: run it once more, by itself, under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/accel_sweep.py
--reps 5` and read DIR/**/run_kernel_stats.csv.
"""
import argparse
import ctypes as C
import importlib
import lzma
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--accels", default="1,2,4,8,16,64")
    ap.add_argument("--only", default="appf64k,book64k,appf4m")
    ap.add_argument("--sample", type=int, default=16, help="blocks per cell checked against the reference library")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 timed launches per cell"
    import torch
    amd = importlib.import_module("lz4-java_amd")
    from oracle import oracle as O
    dev = torch.device("cuda:0")
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    accels = [int(a) for a in args.accels.split(",")]
    ref_fast = None
    if O.ref_path():
        f = C.CDLL(O.ref().path).LZ4_compress_fast
        f.restype = C.c_int
        f.argtypes = [C.c_char_p, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int]

        def ref_fast(v, a):
            cap = len(v) + len(v) // 255 + 16
            out = (C.c_uint8 * cap)()
            r = f(v, out, len(v), cap, a)
            return bytes(out[:r])

    def workload(name):
        if name == "appf64k":
            n, blk = 65536, 65536
            src = torch.empty(n * blk, dtype=u8, device=dev)
            amd.DeviceBatch.gen_blocks(src, blk, blk, n)
        elif name == "book64k":
            n, blk = 8192, 65536
            book = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "calgary", "book1.xz"), "rb").read())
            rng = random.Random(0xB00C1)
            host = bytearray(n * blk)
            for i in range(n):
                o = rng.randrange(len(book) - blk)
                host[i * blk:(i + 1) * blk] = book[o:o + blk]
            src = torch.frombuffer(host, dtype=u8).to(dev)
        else:
            n, blk = 1024, 4 << 20
            src = torch.empty(n * blk, dtype=u8, device=dev)
            amd.DeviceBatch.gen_blocks(src, blk, blk, n, first_idx=1 << 24, win=4096)
        torch.cuda.synchronize()
        return n, blk, src

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# accel_sweep: LZ4_compress_fast(..., acceleration) on %s, %d timed launches per cell (median, min .. max GB/s of input)"
         % (torch.cuda.get_device_name(0), args.reps))
    emit("%-8s %6s %10s %18s %8s %10s %8s %s" % ("workload", "accel", "GB/s", "spread", "ratio", "vs first", "decode", "reference"))
    for name in args.only.split(","):
        n, blk, src = workload(name)
        cap = blk + blk // 255 + 16
        so = torch.arange(n, dtype=i64, device=dev) * blk
        sl = torch.full((n,), blk, dtype=i32, device=dev)
        co = torch.arange(n, dtype=i64, device=dev) * cap
        cc = torch.full((n,), cap, dtype=i32, device=dev)
        clen = torch.zeros(n, dtype=i32, device=dev)
        dlen = torch.zeros(n, dtype=i32, device=dev)
        comp = torch.empty(n * cap, dtype=u8, device=dev)
        base = None
        for a in accels:
            run = lambda: amd.DeviceBatch.compress_fast(src, so, sl, comp, co, cc, clen, acceleration=a)
            run()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e-3)
            gbs = sorted(n * blk / t / 1e9 for t in ts)
            med = gbs[len(gbs) // 2]
            sizes = clen.cpu()
            ok_sizes = bool((sizes > 0).all())
            ratio = n * blk / float(sizes.to(i64).sum())
            back = torch.zeros(n * blk, dtype=u8, device=dev)
            amd.DeviceBatch.decompress_safe(comp, co, clen, back, so, sl, dlen)
            torch.cuda.synchronize()
            rt = ok_sizes and bool((dlen == blk).all()) and torch.equal(back, src)
            del back
            refs = "n/a"
            if ref_fast is not None and args.sample:
                idx = random.Random(a * 1000 + n).sample(range(n), min(args.sample, n))
                good = sum(comp[i * cap:i * cap + int(sizes[i])].cpu().numpy().tobytes() == ref_fast(src[i * blk:(i + 1) * blk].cpu().numpy().tobytes(), a)
                           for i in idx)
                refs = "%d/%d bit-exact" % (good, len(idx))
            if a == accels[0]:
                base = med
            emit("%-8s %6d %10.1f %18s %8.3f %10s %8s %s" % (name, a, med, "%.1f .. %.1f" % (gbs[0], gbs[-1]), ratio,
                                                             "%.2fx" % (med / base), "ok" if rt else "FAILED", refs))
        del src, comp
        torch.cuda.empty_cache()
    emit("# (vs first: median GB/s relative to the first acceleration of the workload)")
    emit("# %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
