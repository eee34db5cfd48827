#!/usr/bin/env python3
"""tools/partial_sweep.py -- throughput of LZ4_decompress_safe_partial (decode a prefix of every block) on one MI355X.

Device-resident workloads (nothing crosses PCIe while timing), compressed on the device by lz4hip_compress_fast first:
  appf64k   65536 x 64 KiB SURVEY.md App. F blocks (DeviceBatch.gen_blocks: the headline's blocks) -> decode_partial_kernel (staged)
  appf8k    8192 x 64 KiB App. F blocks                                                            -> decode_partial_deep_kernel
  book64k   65536 x 64 KiB slices of Calgary book1 (tests/golden/calgary/book1.xz, seeded offsets)  -> decode_partial_kernel
  appf4m    1024 x 4 MiB App. F blocks, win 4096                                                   -> decode_partial_deep_kernel
  single    one 64 KiB App. F block through the single call (lz4hip_decompress_safe_partial, host pointers, coalescing combiner)
Targets: 1 KiB, 4 KiB, 16 KiB and the whole block; every block of a cell has the same target and capacity = the block size.

Per cell: one warm-up launch, then --reps timed launches, each between its own pair of HIP events on torch's stream; reported: GB/s of
DECODED output of the median launch (sum of out_len / time) and its spread; lz4hip_decompress_safe_batch_dev on the same batch (the
whole blocks, output GB/s and time of its median launch: the time a caller who needs the prefix pays without this call); the reference
library's LZ4_decompress_safe_partial on --threads host threads over the first --ref-blocks blocks (decoded GB/s, best of three passes
of tools/partial_refbench.c: pthreads over the dlopen'd library); and the return values and bytes of a seeded sample of blocks
against it.  The single-call row reports the median of --single-calls calls (microseconds) next to lz4hip_decompress_safe's.

  python tools/partial_sweep.py [--reps 7] [--out profiles/partial_sweep.txt] [--only appf64k,appf8k,book64k,appf4m,single]
Kernel times: run it once more, by itself, under `rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python
tools/partial_sweep.py --reps 5 --sample 0 --ref-blocks 0` and read DIR/**/run_kernel_stats.csv.
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
TARGETS = (1024, 4096, 16384, 0)   # 0 = the whole block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="appf64k,appf8k,book64k,appf4m,single")
    ap.add_argument("--sample", type=int, default=16, help="blocks per cell checked against the reference library")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the reference's LZ4_decompress_safe_partial")
    ap.add_argument("--ref-blocks", type=int, default=4096, help="blocks of a cell the reference decodes (0 = none)")
    ap.add_argument("--single-calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 timed launches per cell"
    import torch
    amd = importlib.import_module("lz4-java_amd")
    from oracle import oracle as O
    dev = torch.device("cuda:0")
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    ref_part = None
    tmp = tempfile.mkdtemp(prefix="partial_sweep_")
    if O.ref_path():
        f = C.CDLL(O.ref().path).LZ4_decompress_safe_partial
        f.restype = C.c_int
        f.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int]

        def ref_part(s, t, cap):
            out = (C.c_uint8 * cap)()
            r = f(s, out, len(s), t, cap)
            return r, bytes(out[:max(r, 0)])

        # the host side runs in C (tools/partial_refbench.c, pthreads): Python threads would measure the interpreter, not liblz4
        refbench = os.path.join(tmp, "partial_refbench")
        subprocess.check_call(["gcc", "-O2", "-o", refbench, os.path.join(ROOT, "tools", "partial_refbench.c"), "-lpthread", "-ldl"])

        def ref_rate(streams, blk, t):
            sp, lp = os.path.join(tmp, "streams.bin"), os.path.join(tmp, "lens.bin")
            with open(sp, "wb") as fh:
                fh.write(b"".join(streams))
            with open(lp, "wb") as fh:
                fh.write(b"".join(len(s).to_bytes(4, "little") for s in streams))
            c, secs = subprocess.check_output([refbench, O.ref().path, sp, lp, str(blk), str(t), str(args.threads)]).split()
            return int(c) / float(secs) / 1e9

    def workload(name):
        if name in ("appf64k", "appf8k", "single"):
            n, blk = {"appf64k": 65536, "appf8k": 8192, "single": 1}[name], 65536
            src = torch.empty(n * blk, dtype=u8, device=dev)
            amd.DeviceBatch.gen_blocks(src, blk, blk, n)
        elif name == "book64k":
            n, blk = 65536, 65536
            book = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "calgary", "book1.xz"), "rb").read())
            rng = random.Random(0xB00C1)
            host = bytearray(n * blk)
            for i in range(n):
                o = rng.randrange(len(book) - blk)
                host[i * blk:(i + 1) * blk] = book[o:o + blk]
            src = torch.frombuffer(host, dtype=u8).to(dev)
            del host
        else:
            n, blk = 1024, 4 << 20
            src = torch.empty(n * blk, dtype=u8, device=dev)
            amd.DeviceBatch.gen_blocks(src, blk, blk, n, first_idx=1 << 24, win=4096)
        so = torch.arange(n, dtype=i64, device=dev) * blk
        sl = torch.full((n,), blk, dtype=i32, device=dev)
        cap = blk + blk // 255 + 16
        co = torch.arange(n, dtype=i64, device=dev) * cap
        cc = torch.full((n,), cap, dtype=i32, device=dev)
        clen = torch.zeros(n, dtype=i32, device=dev)
        comp = torch.empty(n * cap, dtype=u8, device=dev)
        amd.DeviceBatch.compress_fast(src, so, sl, comp, co, cc, clen)
        torch.cuda.synchronize()
        del src
        return n, blk, comp, co, clen

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

    emit("# partial_sweep: LZ4_decompress_safe_partial on %s, %d timed launches per cell (median, min .. max GB/s of DECODED output)"
         % (torch.cuda.get_device_name(0), args.reps))
    emit("%-8s %7s %8s %10s %16s %9s %10s %10s %9s %8s %s" % ("workload", "blocks", "target", "GB/s", "spread", "ms", "full GB/s", "full ms",
                                                           "ref GB/s", "vs ref", "reference"))
    for name in args.only.split(","):
        n, blk, comp, co, clen = workload(name)
        streams = None
        if ref_part is not None and (args.sample or args.ref_blocks or name == "single"):
            nh = max(min(n, args.ref_blocks), min(n, args.sample))
            ch, lh = comp.cpu().numpy(), clen.cpu().numpy()
            cap = blk + blk // 255 + 16
            streams = [ch[i * cap:i * cap + int(lh[i])].tobytes() for i in range(nh)]
            del ch
        do = torch.arange(n, dtype=i64, device=dev) * blk
        dc = torch.full((n,), blk, dtype=i32, device=dev)
        dst = torch.empty(n * blk, dtype=u8, device=dev)
        out = torch.zeros(n, dtype=i32, device=dev)
        if name == "single":
            L = amd.lib()
            s = streams[0]
            hd = (C.c_uint8 * blk)()

            def per_call(fn):
                fn()
                ts = []
                for _ in range(args.single_calls):
                    t0 = time.perf_counter()
                    fn()
                    ts.append(time.perf_counter() - t0)
                return sorted(ts)[len(ts) // 2]
            full = per_call(lambda: L.lz4hip_decompress_safe(s, len(s), hd, blk))
            for t in TARGETS:
                tt = t or blk
                med = per_call(lambda: L.lz4hip_decompress_safe_partial(s, len(s), hd, tt, blk))
                r = L.lz4hip_decompress_safe_partial(s, len(s), hd, tt, blk)
                good = (r, bytes(hd[:max(r, 0)])) == ref_part(s, tt, blk)
                emit("%-8s %7d %8d %10.3f %16s %9.3f %10.3f %10.3f %9s %8s %s" % (name, n, tt, tt / med / 1e9, "(per call)", med * 1e3,
                                                                              blk / full / 1e9, full * 1e3, "n/a", "n/a",
                                                                              "1/1 bit-exact" if good else "0/1 bit-exact"))
            continue
        tf = timed(lambda: amd.DeviceBatch.decompress_safe(comp, co, clen, dst, do, dc, out), args.reps)
        full_ms = tf[len(tf) // 2] * 1e3
        full = n * blk / tf[len(tf) // 2] / 1e9
        for t in TARGETS:
            tt = t or blk
            tl = torch.full((n,), tt, dtype=i32, device=dev)
            ts = timed(lambda: amd.DeviceBatch.decompress_safe_partial(comp, co, clen, dst, do, tl, dc, out), args.reps)
            decoded = float(out.to(i64).sum())
            gbs = sorted(decoded / x / 1e9 for x in ts)
            med = gbs[len(gbs) // 2]
            refs, rr, vs = "n/a", "n/a", "n/a"
            if streams is not None:
                if args.sample:
                    idx = random.Random(tt * 7 + n).sample(range(len(streams)), min(args.sample, len(streams)))
                    oh = out.cpu().numpy()
                    good = 0
                    for i in idx:
                        r, b = ref_part(streams[i], tt, blk)
                        good += int(oh[i]) == r and dst[i * blk:i * blk + max(r, 0)].cpu().numpy().tobytes() == b
                    refs = "%d/%d bit-exact" % (good, len(idx))
                if args.ref_blocks:
                    r = ref_rate(streams[:min(n, args.ref_blocks)], blk, tt)
                    rr, vs = "%.2f" % r, "%.1fx" % (med / r)
            emit("%-8s %7d %8d %10.1f %16s %9.3f %10.1f %10.3f %9s %8s %s" % (name, n, tt, med, "%.1f .. %.1f" % (gbs[0], gbs[-1]),
                                                                          ts[len(ts) // 2] * 1e3, full, full_ms, rr, vs, refs))
        del comp, dst, streams
        torch.cuda.empty_cache()
    emit("# GB/s = sum(out_len) / time; ms = the median launch; full = lz4hip_decompress_safe_batch_dev on the same batch (whole blocks);")
    emit("# ref GB/s = the reference's LZ4_decompress_safe_partial on %d host threads over the first %d blocks of the cell, decoded GB/s;"
         % (args.threads, args.ref_blocks))
    emit("# single: one block per call from the host, GB/s = target / median call time, ms = median call, full = lz4hip_decompress_safe")
    emit("# %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
