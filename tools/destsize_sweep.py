#!/usr/bin/env python3
"""tools/destsize_sweep.py -- throughput of LZ4_compress_destSize (compress to a target size) on one MI355X.

Device-resident workloads (nothing crosses PCIe while timing):
  appf64k   65536 x 64 KiB SURVEY.md App. F blocks (DeviceBatch.gen_blocks: the headline's blocks) at targets 4 KiB, 16 KiB,
            32 KiB and compressBound (65809 bytes: the default bytes, all of the input)
  book64k   8192 x 64 KiB slices of Calgary book1 (tests/golden/calgary/book1.xz, seeded offsets) at 16 KiB
  appf4m    1024 x 4 MiB App. F blocks, win 4096 (byU32 tables) at 1 MiB
Every block of a cell has the same target.  The kernel is compress_fast_dest_cu_kernel (DeviceBatch.compress_dest_size).

Per cell: one warm-up launch, then --reps timed launches, each between its own pair of HIP events on torch's stream; reported: GB/s of
CONSUMED input of the median launch (sum of src_consumed / time) and its spread, the output fill (sum of out_len / sum of targets),
the ratio (consumed / written), lz4hip_compress_fast on the same blocks (input GB/s, median of --reps launches), and -- where the
reference library is on the box -- its LZ4_compress_destSize on --threads host threads over the first --ref-blocks blocks of the
cell (consumed GB/s, best of three passes of tools/destsize_refbench.c: pthreads over the dlopen'd library), and the bytes and
consumed sizes of a seeded sample of blocks against it.

  python tools/destsize_sweep.py [--reps 7] [--out profiles/destsize_sweep.txt] [--only appf64k,book64k,appf4m]
Kernel times: run it once more, by itself, under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/destsize_sweep.py
--reps 5 --sample 0 --ref-blocks 0` (with --output-format csv) and read DIR/**/run_kernel_stats.csv.
"""
import argparse
import ctypes as C
import importlib
import lzma
import os
import random
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CELLS = {"appf64k": (4096, 16384, 32768, 65809), "book64k": (16384,), "appf4m": (1 << 20,)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="appf64k,book64k,appf4m")
    ap.add_argument("--sample", type=int, default=16, help="blocks per cell checked against the reference library")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the reference's LZ4_compress_destSize")
    ap.add_argument("--ref-blocks", type=int, default=4096, help="blocks of a cell the reference compresses (0 = none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 timed launches per cell"
    import torch
    amd = importlib.import_module("lz4-java_amd")
    from oracle import oracle as O
    dev = torch.device("cuda:0")
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    ref_dest = None
    if O.ref_path():
        f = C.CDLL(O.ref().path).LZ4_compress_destSize
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int]

        def ref_dest(v, t):
            out = (C.c_uint8 * t)()
            sz = C.c_int(len(v))
            r = f(v, out, C.byref(sz), t)
            return bytes(out[:r]), sz.value

        # the host side runs in C (tools/destsize_refbench.c, pthreads): Python threads would measure the interpreter, not liblz4
        tmp = tempfile.mkdtemp(prefix="destsize_sweep_")
        refbench = os.path.join(tmp, "destsize_refbench")
        subprocess.check_call(["gcc", "-O2", "-o", refbench, os.path.join(ROOT, "tools", "destsize_refbench.c"), "-lpthread", "-ldl"])

        def ref_rate(host, n, blk, t):
            """consumed GB/s of the reference over blocks [0, n) of `host` on args.threads threads (best of 3 passes)"""
            path = os.path.join(tmp, "blocks.bin")
            with open(path, "wb") as fh:
                fh.write(host[:n * blk])
            c, secs = subprocess.check_output([refbench, O.ref().path, path, str(blk), str(t), str(args.threads)]).split()
            return int(c) / float(secs) / 1e9

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

    def timed(run, reps):
        run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        return sorted(ts)

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# destsize_sweep: LZ4_compress_destSize on %s, %d timed launches per cell (median, min .. max GB/s of CONSUMED input)"
         % (torch.cuda.get_device_name(0), args.reps))
    emit("%-8s %8s %10s %16s %7s %7s %10s %12s %8s %s" % ("workload", "target", "GB/s", "spread", "fill", "ratio", "fast GB/s",
                                                          "ref GB/s", "vs ref", "reference"))
    for name in args.only.split(","):
        n, blk, src = workload(name)
        so = torch.arange(n, dtype=i64, device=dev) * blk
        sl = torch.full((n,), blk, dtype=i32, device=dev)
        cap = blk + blk // 255 + 16
        co = torch.arange(n, dtype=i64, device=dev) * cap
        cc = torch.full((n,), cap, dtype=i32, device=dev)
        clen = torch.zeros(n, dtype=i32, device=dev)
        comp = torch.empty(n * cap, dtype=u8, device=dev)
        tf = timed(lambda: amd.DeviceBatch.compress_fast(src, so, sl, comp, co, cc, clen), args.reps)
        fast = n * blk / tf[len(tf) // 2] / 1e9
        host = None
        if ref_dest is not None and (args.sample or args.ref_blocks):
            nh = max(min(n, args.ref_blocks), min(n, args.sample))
            host = src[:nh * blk].cpu().numpy().tobytes()
        for t in CELLS[name]:
            do = torch.arange(n, dtype=i64, device=dev) * t
            ts_ = torch.full((n,), t, dtype=i32, device=dev)
            out = torch.zeros(n, dtype=i32, device=dev)
            cons = torch.zeros(n, dtype=i32, device=dev)
            dst = torch.empty(n * t, dtype=u8, device=dev)
            ts = timed(lambda: amd.DeviceBatch.compress_dest_size(src, so, sl, dst, do, ts_, out, cons), args.reps)
            consumed = float(cons.to(i64).sum())
            written = float(out.to(i64).sum())
            gbs = sorted(consumed / x / 1e9 for x in ts)
            med = gbs[len(gbs) // 2]
            refs, rr, vs = "n/a", "n/a", "n/a"
            if host is not None:
                if args.sample:
                    idx = random.Random(t * 7 + n).sample(range(min(n, len(host) // blk)), min(args.sample, len(host) // blk))
                    oh, ch = out.cpu().numpy(), cons.cpu().numpy()
                    good = 0
                    for i in idx:
                        b, c = ref_dest(host[i * blk:(i + 1) * blk], t)
                        good += int(ch[i]) == c and dst[i * t:i * t + int(oh[i])].cpu().numpy().tobytes() == b
                    refs = "%d/%d bit-exact" % (good, len(idx))
                if args.ref_blocks:
                    r = ref_rate(host, min(n, args.ref_blocks), blk, t)
                    rr, vs = "%.2f" % r, "%.1fx" % (med / r)
            emit("%-8s %8d %10.1f %16s %7.3f %7.3f %10.1f %12s %8s %s" % (name, t, med, "%.1f .. %.1f" % (gbs[0], gbs[-1]),
                                                                          written / (n * t), consumed / written, fast, rr, vs, refs))
            del dst
        del src, comp, host
        torch.cuda.empty_cache()
    emit("# fill = sum(out_len) / sum(target); ratio = consumed / written; fast GB/s = lz4hip_compress_fast, input GB/s, same blocks;")
    emit("# ref GB/s = the reference's LZ4_compress_destSize on %d host threads over the first %d blocks of the cell, consumed GB/s"
         % (args.threads, args.ref_blocks))
    emit("# %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    if ref_dest is not None:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
