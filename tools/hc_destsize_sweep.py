#!/usr/bin/env python3
"""tools/hc_destsize_sweep.py -- throughput of LZ4_compress_HC_destSize (HC compress to a target size) on one MI355X.

Device-resident workloads (nothing crosses PCIe while timing):
  appf64k   16384 x 64 KiB SURVEY.md App. F blocks (DeviceBatch.gen_blocks: the headline's blocks)
  book64k   4096 x 64 KiB slices of Calgary book1 (tests/golden/calgary/book1.xz, seeded offsets)
  appf1m    1024 x 1 MiB App. F blocks, win 4096
at targets 4 KiB, 16 KiB, 32 KiB and whole-block (compressBound of the block: all of the input) and levels 1, 4, 9 and 10 (level 10,
the optimal parser, on the first quarter of each workload's blocks).  Every block of a cell has the same target.  The kernels are
hc_build_kernel + hc_parse_dest_kernel (DeviceBatch.compress_hc_dest_size: the caller's workspace, no synchronisation).

Per cell: one warm-up launch, then --reps timed launches, each between its own pair of HIP events on torch's stream; reported: GB/s of
CONSUMED input of the median launch (sum of src_consumed / time) and its spread, the median launch time, the output fill (sum of
out_len / sum of targets), and two baselines:
  hc GB/s    this project's own lz4hip_compress_hc_batch_dev_ws (DeviceBatch.compress_hc) at the same level on the same blocks, input
             GB/s and launch time, median of --reps launches
  ref GB/s   the reference library's LZ4_compress_HC_destSize on --threads host threads over the first --ref-blocks MiB of the cell
             (consumed GB/s, best of three passes of tools/hc_destsize_refbench.c: pthreads over the dlopen'd library); and the bytes
             and consumed sizes of a seeded sample of blocks against it.
Per workload and level, a launch with every target = 1 is timed too: its parse ends at once, so its time is hc_build_kernel over the
whole blocks plus two launches ("build ms").

  python tools/hc_destsize_sweep.py [--reps 5] [--out profiles/hc_destsize_sweep.txt] [--only appf64k,book64k,appf1m] [--levels 1,4,9,10]
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
SHAPES = {"appf64k": (16384, 65536), "book64k": (4096, 65536), "appf1m": (1024, 1 << 20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="appf64k,book64k,appf1m")
    ap.add_argument("--levels", default="1,4,9,10")
    ap.add_argument("--sample", type=int, default=8, help="blocks per cell checked against the reference library")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the reference's LZ4_compress_HC_destSize")
    ap.add_argument("--ref-mib", type=int, default=64, help="MiB of a cell's blocks the reference compresses (0 = none)")
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
        lib = C.CDLL(O.ref().path)
        f = lib.LZ4_compress_HC_destSize
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int]
        lib.LZ4_sizeofStateHC.restype = C.c_int
        state = C.create_string_buffer(lib.LZ4_sizeofStateHC() + 64)

        def ref_dest(v, t, level):
            out = (C.c_uint8 * t)()
            sz = C.c_int(len(v))
            r = f((C.addressof(state) + 15) & ~15, v, out, C.byref(sz), t, level)
            return bytes(out[:r]), sz.value

        # the host side runs in C (tools/hc_destsize_refbench.c, pthreads): Python threads would measure the interpreter, not liblz4
        tmp = tempfile.mkdtemp(prefix="hc_destsize_sweep_")
        refbench = os.path.join(tmp, "hc_destsize_refbench")
        subprocess.check_call(["gcc", "-O2", "-o", refbench, os.path.join(ROOT, "tools", "hc_destsize_refbench.c"), "-lpthread", "-ldl"])

        def ref_rate(path, blk, t, level):
            """consumed GB/s of the reference over the blocks of the file `path` on args.threads threads (best of 3 passes)"""
            c, secs = subprocess.check_output([refbench, O.ref().path, path, str(blk), str(t), str(args.threads), str(level)]).split()
            return int(c) / float(secs) / 1e9

    def workload(name):
        n, blk = SHAPES[name]
        if name == "book64k":
            book = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "calgary", "book1.xz"), "rb").read())
            rng = random.Random(0xB00C1)
            host = bytearray(n * blk)
            for i in range(n):
                o = rng.randrange(len(book) - blk)
                host[i * blk:(i + 1) * blk] = book[o:o + blk]
            src = torch.frombuffer(host, dtype=u8).to(dev)
        else:
            src = torch.empty(n * blk, dtype=u8, device=dev)
            if name == "appf64k":
                amd.DeviceBatch.gen_blocks(src, blk, blk, n)
            else:
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

    emit("# hc_destsize_sweep: LZ4_compress_HC_destSize on %s, %d timed launches per cell (median, min .. max GB/s of CONSUMED input)"
         % (torch.cuda.get_device_name(0), args.reps))
    emit("%-8s %5s %6s %8s %8s %14s %8s %6s %9s %8s %8s %9s %7s %s" % ("workload", "level", "blocks", "target", "GB/s", "spread", "ms", "fill",
                                                                      "build ms", "hc GB/s", "hc ms", "ref GB/s", "vs ref", "reference"))
    for name in args.only.split(","):
        n_all, blk, src_all = workload(name)
        cap = blk + blk // 255 + 16
        nh = 0
        if ref_dest is not None and (args.sample or args.ref_mib):
            nh = max(1, min(n_all // 4, max(args.ref_mib, 1) * (1 << 20) // blk))
            host = src_all[:nh * blk].cpu().numpy().tobytes()
            if args.ref_mib:
                ref_file = os.path.join(tmp, "blocks.bin")
                with open(ref_file, "wb") as fh:
                    fh.write(host)
        for level in [int(x) for x in args.levels.split(",")]:
            n = n_all // 4 if level >= 10 else n_all
            src = src_all[:n * blk]
            so = torch.arange(n, dtype=i64, device=dev) * blk
            sl = torch.full((n,), blk, dtype=i32, device=dev)
            co = torch.arange(n, dtype=i64, device=dev) * cap
            cc = torch.full((n,), cap, dtype=i32, device=dev)
            clen = torch.zeros(n, dtype=i32, device=dev)
            comp = torch.empty(n * cap, dtype=u8, device=dev)
            th = timed(lambda: amd.DeviceBatch.compress_hc(src, so, sl, comp, co, cc, clen, level), args.reps)
            hc_ms = th[len(th) // 2] * 1e3
            hc = n * blk / th[len(th) // 2] / 1e9
            out = torch.zeros(n, dtype=i32, device=dev)
            cons = torch.zeros(n, dtype=i32, device=dev)
            one = torch.ones(n, dtype=i32, device=dev)
            tb = timed(lambda: amd.DeviceBatch.compress_hc_dest_size(src, so, sl, comp, co, one, out, cons, level), args.reps)
            build_ms = tb[len(tb) // 2] * 1e3
            for t in (4096, 16384, 32768, cap):
                do = torch.arange(n, dtype=i64, device=dev) * t
                ts_ = torch.full((n,), t, dtype=i32, device=dev)
                dst = comp[:n * t]
                ts = timed(lambda: amd.DeviceBatch.compress_hc_dest_size(src, so, sl, dst, do, ts_, out, cons, level), args.reps)
                consumed = float(cons.to(i64).sum())
                written = float(out.to(i64).sum())
                gbs = sorted(consumed / x / 1e9 for x in ts)
                med = gbs[len(gbs) // 2]
                refs, rr, vs = "n/a", "n/a", "n/a"
                if nh:
                    if args.sample:
                        idx = random.Random(t * 7 + n + level).sample(range(nh), min(args.sample, nh))
                        oh, ch = out.cpu().numpy(), cons.cpu().numpy()
                        good = 0
                        for i in idx:
                            b, c = ref_dest(host[i * blk:(i + 1) * blk], t, level)
                            good += int(ch[i]) == c and dst[i * t:i * t + int(oh[i])].cpu().numpy().tobytes() == b
                        refs = "%d/%d bit-exact" % (good, len(idx))
                    if args.ref_mib:
                        r = ref_rate(ref_file, blk, t, level)
                        rr, vs = "%.2f" % r, "%.1fx" % (med / r)
                emit("%-8s %5d %6d %8d %8.2f %14s %8.2f %6.3f %9.2f %8.2f %8.2f %9s %7s %s" % (
                    name, level, n, t, med, "%.2f .. %.2f" % (gbs[0], gbs[-1]), ts[len(ts) // 2] * 1e3, written / (n * t), build_ms, hc, hc_ms, rr,
                    vs, refs))
            del comp
        del src_all
        torch.cuda.empty_cache()
    emit("# GB/s = sum(src_consumed) / launch time; ms = the median launch; fill = sum(out_len) / sum(target); build ms = the same launch with")
    emit("# every target = 1 (hc_build_kernel over the whole blocks, a parse that ends at once); hc GB/s, hc ms = lz4hip_compress_hc_batch_dev_ws,")
    emit("# same level and blocks, input GB/s; ref GB/s = the reference's LZ4_compress_HC_destSize on %d host threads over the first %d MiB"
         % (args.threads, args.ref_mib))
    emit("# of the cell's blocks, consumed GB/s; level 10 runs on the first quarter of the blocks")
    emit("# %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    if ref_dest is not None:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
