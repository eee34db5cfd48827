#!/usr/bin/env python3
"""tools/dict_compress_sweep.py -- throughput of the dictionary compressor (LZ4_loadDict + LZ4_compress_fast_continue on a fresh stream
per record, lz4hip_compress_fast_dict_batch_dev) on one MI355X.

Cells: records of 256 B / 1 KiB / 4 KiB / 64 KiB x dictionaries of 0 / 4 KiB / 64 KiB x 2048 and 65536 records, device-resident
(nothing crosses PCIe while timing).  The records are slices of Calgary book1 (tests/golden/calgary/book1.xz) behind byte 200000 at
seeded offsets, the dictionary is book1's first bytes; a pool of --pool distinct records per cell is repeated on the device until the
cell's record count is reached -- every record has its own copy of its bytes and its own destination slot of compressBound bytes.

Per cell: one warm-up launch (the first one of a dictionary also builds its table image), then --reps timed launches, each between its
own pair of HIP events on torch's stream; reported as GB/s of SOURCE bytes of the median launch (and min .. max):
  dict      compress_fast_dict_cu_kernel against the dictionary
  plain     lz4hip_compress_fast_batch_dev on the same records without a dictionary, as context: what the engine's default compressor
            does on records of this size
  size      compressed bytes with the dictionary / compressed bytes of `plain`: what the dictionary buys
  ref       the reference library's LZ4_loadDict + LZ4_compress_fast_continue on --threads host threads over the first --ref-blocks
            records (tools/dict_compress_refbench.c: pthreads over the dlopen'd library, best of three passes)
and the return values and bytes of a seeded sample of records against the reference.

  python tools/dict_compress_sweep.py [--reps 7] [--out profiles/dict_compress_sweep.txt]
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
RECORDS = (256, 1024, 4096, 65536)
DICTS = (0, 4096, 65536)
BLOCKS = (2048, 65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pool", type=int, default=2048, help="distinct records per cell")
    ap.add_argument("--sample", type=int, default=32, help="records per cell checked against the reference library")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the reference")
    ap.add_argument("--ref-blocks", type=int, default=4096, help="records of a cell the reference compresses (0 = none)")
    ap.add_argument("--records", default=",".join(map(str, RECORDS)))
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
    R.LZ4_createStream.restype = C.c_void_p
    R.LZ4_freeStream.argtypes = [C.c_void_p]
    R.LZ4_loadDict.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    R.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    tmp = tempfile.mkdtemp(prefix="dict_compress_sweep_")
    refbench = os.path.join(tmp, "dict_compress_refbench")
    subprocess.check_call(["gcc", "-O2", "-o", refbench, os.path.join(ROOT, "tools", "dict_compress_refbench.c"), "-lpthread", "-ldl"])

    def ref_compress(dbuf, dlen, rec):
        out = C.create_string_buffer(len(rec) + len(rec) // 255 + 64)
        st = R.LZ4_createStream()
        R.LZ4_loadDict(st, dbuf, dlen)
        n = R.LZ4_compress_fast_continue(st, rec, out, len(rec), len(out), 1)
        R.LZ4_freeStream(st)
        assert n > 0
        return out.raw[:n]

    def ref_rate(recs, rec, dpath):
        rp = os.path.join(tmp, "records.bin")
        with open(rp, "wb") as fh:
            fh.write(b"".join(recs))
        src_bytes, _, secs = subprocess.check_output([refbench, ref.path, dpath, rp, str(rec), str(args.threads)]).split()
        return int(src_bytes) / float(secs) / 1e9

    def timed(run):
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
        return sorted(ts)

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# dict_compress_sweep: LZ4_loadDict + LZ4_compress_fast_continue on %s, %d timed launches per cell (median, min .. max GB/s of SOURCE bytes)"
         % (torch.cuda.get_device_name(0), args.reps))
    emit("%7s %6s %7s %6s %9s %16s %8s %9s %6s %9s %8s %s" % ("record", "dict", "blocks", "ratio", "dict GB/s", "spread", "ms", "plain", "size",
                                                              "ref GB/s", "vs ref", "reference"))
    for rec in [int(x) for x in args.records.split(",")]:
        rng = random.Random(0xD1C7 + rec)
        pool = min(args.pool, 2048)
        recs = []
        for _ in range(pool):
            o = rng.randrange(200000, len(book) - rec)
            recs.append(book[o:o + rec])
        cap = rec + rec // 255 + 16
        pool_t = torch.from_numpy(np.frombuffer(b"".join(recs), dtype=np.uint8).copy()).to(dev)
        for dlen in DICTS:
            d = book[:dlen]
            dbuf = C.create_string_buffer(d, max(dlen, 1))
            dpath = os.path.join(tmp, "dict.bin")
            with open(dpath, "wb") as fh:
                fh.write(d)
            ref_gbs = ref_rate((recs * max(1, args.ref_blocks // pool))[:max(args.ref_blocks, 1)], rec, dpath) if args.ref_blocks else None
            with amd.LZ4Dictionary(d) as handle:
                for n in BLOCKS:
                    reps = (n + pool - 1) // pool
                    src = torch.cat([pool_t.repeat(reps)[:n * rec], torch.zeros(64, dtype=u8, device=dev)])
                    so = torch.arange(n, dtype=i64, device=dev) * rec
                    sl = torch.full((n,), rec, dtype=i32, device=dev)
                    do = torch.arange(n, dtype=i64, device=dev) * cap
                    dc = torch.full((n,), cap, dtype=i32, device=dev)
                    dst = torch.empty(n * cap + 64, dtype=u8, device=dev)
                    out = torch.zeros(n, dtype=i32, device=dev)
                    ts = timed(lambda: amd.DeviceBatch.compress_dict(src, so, sl, dst, do, dc, out, handle))
                    oh = out.cpu().numpy()
                    assert (oh > 0).all(), "a record of the cell did not compress"
                    size_dict = float(oh.astype(np.int64).sum())
                    gbs = sorted(float(n) * rec / x / 1e9 for x in ts)
                    med = gbs[len(gbs) // 2]
                    good, idx = 0, random.Random(n + rec).sample(range(n), min(args.sample, n))
                    for i in idx:
                        by = ref_compress(dbuf, dlen, recs[i % pool])
                        good += int(oh[i]) == len(by) and dst[i * cap:i * cap + len(by)].cpu().numpy().tobytes() == by
                    tp = timed(lambda: amd.DeviceBatch.compress_fast(src, so, sl, dst, do, dc, out))
                    size_plain = float(out.to(i64).sum())
                    plain = float(n) * rec / tp[len(tp) // 2] / 1e9
                    emit("%7d %6d %7d %6.3f %9.1f %16s %8.3f %9.1f %6.3f %9s %8s %s"
                         % (rec, dlen, n, size_dict / (float(n) * rec), med, "%.1f .. %.1f" % (gbs[0], gbs[-1]), ts[len(ts) // 2] * 1e3, plain,
                            size_dict / size_plain, "%.2f" % ref_gbs if ref_gbs else "n/a", "%.1fx" % (med / ref_gbs) if ref_gbs else "n/a",
                            "%d/%d bit-exact" % (good, len(idx))))
                    del src, dst
                    torch.cuda.empty_cache()
    emit("# GB/s = records x record bytes / time of the median launch; ratio = compressed / raw bytes with the dictionary; plain =")
    emit("# lz4hip_compress_fast_batch_dev on the same records; size = compressed bytes with the dictionary / compressed bytes of plain;")
    emit("# ref = the reference's LZ4_loadDict + LZ4_compress_fast_continue, a fresh stream per record, on %d host threads over %d records,"
         % (args.threads, args.ref_blocks))
    emit("# source GB/s (best of three passes)")
    emit("# %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
