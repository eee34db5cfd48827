#!/usr/bin/env python3
"""tools/hc_dict_sweep.py -- throughput of the dictionary HC compressor (LZ4_loadDictHC + LZ4_compress_HC_continue on a fresh stream
per record, lz4hip_compress_hc_dict_batch_dev_ws) on one MI355X.

Cells: levels 1 / 4 / 9 / 10 x 65536 records of 1 KiB, 16384 of 4 KiB and 4096 of 64 KiB cut from Calgary book1
(tests/golden/calgary/book1.xz) behind byte 200000 at seeded offsets, plus 4096 SURVEY.md App. F blocks of 64 KiB, x dictionaries of
4 KiB and 64 KiB (book1's first bytes), device-resident (nothing crosses PCIe while timing).  A pool of distinct records per cell is
repeated on the device until the cell's record count is reached; every record has its own copy of its bytes and its own slot of
compressBound bytes.  The chain workspace is allocated once per cell, outside the timed region.

Per cell: one warm-up launch (a dictionary's first one also builds its image), then --reps timed launches, each between its own pair
of HIP events on torch's stream; reported as GB/s of SOURCE bytes of the median launch (and min .. max):
  dict      hc_build_dict_kernel + hc_parse_dict_kernel against the dictionary
  hc        lz4hip_compress_hc_batch_dev_ws at the same level on the same records without a dictionary
  size      compressed bytes with the dictionary / compressed bytes of `hc`: what the dictionary buys
  build     the same two launches with every capacity 0: the parse stops at its first sequence, so the launch is the delta[] build --
            with the dictionary (the 128 KB head-table load per record) and without (the zero fill)
  ref       the reference library's three calls on --threads host threads over the first records of the cell, at most --ref-mib MiB
            (tools/hc_dict_refbench.c: pthreads over the dlopen'd library, best of three passes)
and the return values and bytes of a seeded sample of records against the reference.

  python tools/hc_dict_sweep.py [--reps 5] [--out profiles/hc_dict_sweep.txt]
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
LEVELS = (1, 4, 9, 10)
CELLS = (("book1", 1024, 65536), ("book1", 4096, 16384), ("book1", 65536, 4096), ("App. F", 65536, 4096))
DICTS = (4096, 65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pool", type=int, default=1024, help="distinct records per cell")
    ap.add_argument("--sample", type=int, default=16, help="records per cell checked against the reference library")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the reference")
    ap.add_argument("--ref-mib", type=int, default=8, help="MiB of a cell's records the reference compresses (0 = none)")
    ap.add_argument("--levels", default=",".join(map(str, LEVELS)))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 timed launches per cell"
    import numpy as np
    import torch
    amd = importlib.import_module("lz4-java_amd")
    from oracle import oracle as O
    dev = torch.device("cuda:0")
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    book = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "calgary", "book1.xz"), "rb").read())
    ref = O.ref()
    R = C.CDLL(ref.path)
    R.LZ4_createStreamHC.restype = C.c_void_p
    R.LZ4_freeStreamHC.argtypes = [C.c_void_p]
    R.LZ4_resetStreamHC_fast.argtypes = [C.c_void_p, C.c_int]
    R.LZ4_loadDictHC.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    R.LZ4_compress_HC_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    tmp = tempfile.mkdtemp(prefix="hc_dict_sweep_")
    refbench = os.path.join(tmp, "hc_dict_refbench")
    subprocess.check_call(["gcc", "-O2", "-o", refbench, os.path.join(ROOT, "tools", "hc_dict_refbench.c"), "-lpthread", "-ldl"])

    def ref_compress(dbuf, dlen, rec, level):
        out = C.create_string_buffer(len(rec) + len(rec) // 255 + 64)
        st = R.LZ4_createStreamHC()
        R.LZ4_resetStreamHC_fast(st, level)
        R.LZ4_loadDictHC(st, dbuf, dlen)
        n = R.LZ4_compress_HC_continue(st, rec, out, len(rec), len(out))
        R.LZ4_freeStreamHC(st)
        assert n > 0
        return out.raw[:n]

    def ref_rate(recs, rec, dpath, level):
        rp = os.path.join(tmp, "records.bin")
        with open(rp, "wb") as fh:
            fh.write(b"".join(recs))
        src_bytes, _, secs = subprocess.check_output([refbench, ref.path, dpath, rp, str(rec), str(args.threads), str(level)]).split()
        return int(src_bytes) / float(secs) / 1e9

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

    emit("# hc_dict_sweep: LZ4_loadDictHC + LZ4_compress_HC_continue on %s, %d timed launches per cell (median, min .. max GB/s of SOURCE bytes)"
         % (torch.cuda.get_device_name(0), args.reps))
    emit("%5s %7s %7s %6s %7s %6s %9s %16s %9s %8s %6s %11s %11s %9s %8s %s"
         % ("level", "records", "record", "dict", "blocks", "ratio", "dict GB/s", "spread", "ms", "hc GB/s", "size", "build dict", "build hc", "ref GB/s",
            "vs ref", "reference"))
    for kind, rec, n in CELLS:
        rng = random.Random(0x4CD1 + rec + len(kind))
        pool = min(args.pool, n)
        if kind == "book1":
            recs = []
            for _ in range(pool):
                o = rng.randrange(200000, len(book) - rec)
                recs.append(book[o:o + rec])
        else:
            pool = min(pool, 256)
            recs = [O.gen_block(rec, i) for i in range(pool)]
        cap = rec + rec // 255 + 16
        pool_t = torch.from_numpy(np.frombuffer(b"".join(recs), dtype=np.uint8).copy()).to(dev)
        src = torch.cat([pool_t.repeat((n + pool - 1) // pool)[:n * rec], torch.zeros(64, dtype=u8, device=dev)])
        so = torch.arange(n, dtype=i64, device=dev) * rec
        sl = torch.full((n,), rec, dtype=i32, device=dev)
        do = torch.arange(n, dtype=i64, device=dev) * cap
        dc = torch.full((n,), cap, dtype=i32, device=dev)
        dc0 = torch.zeros(n, dtype=i32, device=dev)
        dst = torch.empty(n * cap + 64, dtype=u8, device=dev)
        out = torch.zeros(n, dtype=i32, device=dev)
        span = n * rec
        for level in [int(x) for x in args.levels.split(",")]:
            nb = amd.lib().lz4hip_hc_workspace_bytes(span, n, level)
            ws = torch.empty(nb, dtype=u8, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream

            def plain(caps):
                amd._chk(amd.lib().lz4hip_compress_hc_batch_dev_ws(src.data_ptr(), so.data_ptr(), sl.data_ptr(), dst.data_ptr(), do.data_ptr(),
                                                                   caps.data_ptr(), out.data_ptr(), n, level, 0, st, span, ws.data_ptr(), nb))

            tp = timed(lambda: plain(dc), args.reps)
            size_plain = float(out.to(i64).sum())
            hc = float(n) * rec / tp[len(tp) // 2] / 1e9
            tb0 = timed(lambda: plain(dc0), 3)
            for dlen in DICTS:
                d = book[:dlen]
                dbuf = C.create_string_buffer(d, max(dlen, 1))
                dpath = os.path.join(tmp, "dict.bin")
                with open(dpath, "wb") as fh:
                    fh.write(d)
                n_ref = min(n, max(1, (args.ref_mib << 20) // rec))
                ref_gbs = ref_rate((recs * ((n_ref + pool - 1) // pool))[:n_ref], rec, dpath, level) if args.ref_mib else None
                with amd.LZ4Dictionary(d) as handle:
                    ts = timed(lambda: amd.DeviceBatch.compress_hc_dict(src, so, sl, dst, do, dc, out, handle, level, span=span, ws=ws), args.reps)
                    oh = out.cpu().numpy()
                    assert (oh > 0).all(), "a record of the cell did not compress"
                    size_dict = float(oh.astype(np.int64).sum())
                    gbs = sorted(float(n) * rec / x / 1e9 for x in ts)
                    med = gbs[len(gbs) // 2]
                    good, idx = 0, random.Random(n + rec).sample(range(n), min(args.sample, n))
                    for i in idx:
                        by = ref_compress(dbuf, dlen, recs[i % pool], level)
                        good += int(oh[i]) == len(by) and dst[i * cap:i * cap + len(by)].cpu().numpy().tobytes() == by
                    tb = timed(lambda: amd.DeviceBatch.compress_hc_dict(src, so, sl, dst, do, dc0, out, handle, level, span=span, ws=ws), 3)
                emit("%5d %7s %7d %6d %7d %6.3f %9.2f %16s %9.3f %8.2f %6.3f %11s %11s %9s %8s %s"
                     % (level, kind, rec, dlen, n, size_dict / (float(n) * rec), med, "%.2f .. %.2f" % (gbs[0], gbs[-1]), ts[len(ts) // 2] * 1e3, hc,
                        size_dict / size_plain, "%.3f ms" % (tb[len(tb) // 2] * 1e3), "%.3f ms" % (tb0[len(tb0) // 2] * 1e3),
                        "%.3f" % ref_gbs if ref_gbs else "n/a", "%.1fx" % (med / ref_gbs) if ref_gbs else "n/a", "%d/%d bit-exact" % (good, len(idx))))
            del ws
        del src, dst
        torch.cuda.empty_cache()
    emit("# GB/s = records x record bytes / time of the median launch; ratio = compressed / raw bytes with the dictionary; hc =")
    emit("# lz4hip_compress_hc_batch_dev_ws at the same level on the same records; size = compressed bytes with the dictionary / compressed")
    emit("# bytes of hc; build = median of 3 launches with every capacity 0 (the parse stops at its first sequence: the delta[] build, with")
    emit("# the 128 KB head-table load per record / with the zero fill); ref = the reference's LZ4_resetStreamHC_fast + LZ4_loadDictHC +")
    emit("# LZ4_compress_HC_continue, a fresh stream per record, on %d host threads over at most %d MiB of the cell's records, source GB/s" % (args.threads, args.ref_mib))
    emit("# (best of three passes)")
    emit("# %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
