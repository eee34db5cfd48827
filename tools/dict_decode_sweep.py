#!/usr/bin/env python3
"""tools/dict_decode_sweep.py -- throughput of the dictionary decoder (LZ4_decompress_safe_usingDict, lz4hip_decompress_safe_dict_batch_dev)
on one MI355X.

Cells: records of 256 B / 1 KiB / 4 KiB / 64 KiB x dictionaries of 4 KiB / 64 KiB x 2048 and 65536 blocks, device-resident (nothing
crosses PCIe while timing).  The records are slices of Calgary book1 (tests/golden/calgary/book1.xz) behind byte 200000 at seeded
offsets, the dictionary is book1's first bytes; a pool of --pool distinct records per cell is compressed on the host by the reference
library (LZ4_loadDict + LZ4_compress_fast_continue, each record alone against the dictionary) and repeated on the device until the
cell's block count is reached -- every block has its own copy of its stream and its own destination slot.

Per cell: one warm-up launch, then --reps timed launches, each between its own pair of HIP events on torch's stream; reported as GB/s
of DECODED output of the median launch (and min .. max):
  dict      the dictionary kernels (2048 blocks: decode_dict_deep_kernel, 65536: decode_dict_kernel)
  exact     the same from a developer build whose interior loops leave every match that starts in the dictionary to the exact path
            (tools/build_variant.sh dict_exact_only -DLZ4HIP_DICT_INTERIOR=0; --variant names the library) -- what taking those
            matches in the interior loops bought
  plain     lz4hip_decompress_safe_batch_dev on the same records compressed WITHOUT a dictionary (LZ4_compress_default), as context:
            what the engine does on records of this size when there is no dictionary (and more compressed bytes)
  ref       the reference library's LZ4_decompress_safe_usingDict on --threads host threads over the first --ref-blocks blocks
            (tools/dict_decode_refbench.c: pthreads over the dlopen'd library, best of three passes)
and the return values and bytes of a seeded sample of blocks against the reference.

  python tools/dict_decode_sweep.py [--reps 7] [--variant lz4-java_amd/variants/dict_exact_only.so] [--out profiles/dict_decode_sweep.txt]
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
DICTS = (4096, 65536)
BLOCKS = (2048, 65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pool", type=int, default=2048, help="distinct records per cell")
    ap.add_argument("--sample", type=int, default=32, help="blocks per cell checked against the reference library")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the reference's LZ4_decompress_safe_usingDict")
    ap.add_argument("--ref-blocks", type=int, default=4096, help="blocks of a cell the reference decodes (0 = none)")
    ap.add_argument("--variant", default=os.path.join(ROOT, "lz4-java_amd", "variants", "dict_exact_only.so"))
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
    R.LZ4_decompress_safe_usingDict.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    tmp = tempfile.mkdtemp(prefix="dict_decode_sweep_")
    refbench = os.path.join(tmp, "dict_decode_refbench")
    subprocess.check_call(["gcc", "-O2", "-o", refbench, os.path.join(ROOT, "tools", "dict_decode_refbench.c"), "-lpthread", "-ldl"])
    variant = None
    if args.variant and os.path.exists(args.variant):
        variant = C.CDLL(args.variant)
        variant.lz4hip_decompress_safe_dict_batch_dev.restype = C.c_int
        variant.lz4hip_decompress_safe_dict_batch_dev.argtypes = amd.C_ABI["lz4hip_decompress_safe_dict_batch_dev"][1]

    def compress_with_dict(dbuf, dlen, rec):
        out = C.create_string_buffer(len(rec) + len(rec) // 255 + 64)
        st = R.LZ4_createStream()
        R.LZ4_loadDict(st, dbuf, dlen)
        n = R.LZ4_compress_fast_continue(st, rec, out, len(rec), len(out), 1)
        R.LZ4_freeStream(st)
        assert n > 0
        return out.raw[:n]

    def ref_decode(s, cap, dbuf, dlen):
        out = (C.c_uint8 * (cap + 64))()
        r = R.LZ4_decompress_safe_usingDict(s, out, len(s), cap, dbuf, dlen)
        return r, bytes(out[:max(r, 0)])

    def ref_rate(streams, rec, dpath):
        sp, lp = os.path.join(tmp, "streams.bin"), os.path.join(tmp, "lens.bin")
        with open(sp, "wb") as fh:
            fh.write(b"".join(streams))
        with open(lp, "wb") as fh:
            fh.write(b"".join(len(s).to_bytes(4, "little") for s in streams))
        c, secs = subprocess.check_output([refbench, ref.path, dpath, sp, lp, str(rec), str(args.threads)]).split()
        return int(c) / float(secs) / 1e9

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

    def batch(streams, n):
        """the pool's streams repeated up to n blocks, on the device: (src, src_off, src_len)"""
        pool = np.frombuffer(b"".join(streams), dtype=np.uint8)
        lens = np.array([len(s) for s in streams], dtype=np.int64)
        reps = (n + len(streams) - 1) // len(streams)
        src = torch.from_numpy(pool.copy()).to(dev).repeat(reps)
        off1 = np.concatenate([[0], np.cumsum(lens)[:-1]])
        off = (off1[None, :] + (np.arange(reps, dtype=np.int64) * len(pool))[:, None]).reshape(-1)[:n]
        sl = np.tile(lens, reps)[:n].astype(np.int32)
        return torch.cat([src, torch.zeros(64, dtype=u8, device=dev)]), torch.from_numpy(off).to(dev), torch.from_numpy(sl).to(dev)

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# dict_decode_sweep: LZ4_decompress_safe_usingDict on %s, %d timed launches per cell (median, min .. max GB/s of DECODED output)"
         % (torch.cuda.get_device_name(0), args.reps))
    emit("%7s %6s %7s %6s %9s %16s %8s %9s %9s %9s %8s %s" % ("record", "dict", "blocks", "ratio", "dict GB/s", "spread", "ms", "exact", "plain",
                                                              "ref GB/s", "vs ref", "reference"))
    for rec in [int(x) for x in args.records.split(",")]:
        rng = random.Random(0xD1C7 + rec)
        pool = min(args.pool, 2048)
        recs = []
        for _ in range(pool):
            o = rng.randrange(200000, len(book) - rec)
            recs.append(book[o:o + rec])
        plain_streams = [ref.compress_fast(r) for r in recs]
        for dlen in DICTS:
            d = book[:dlen]
            dbuf = C.create_string_buffer(d, dlen)
            dpath = os.path.join(tmp, "dict.bin")
            with open(dpath, "wb") as fh:
                fh.write(d)
            streams = [compress_with_dict(dbuf, dlen, r) for r in recs]
            ratio = sum(len(s) for s in streams) / float(rec * pool)
            dict_t = torch.frombuffer(bytearray(d), dtype=u8).to(dev)
            ref_gbs = ref_rate(streams[:min(pool, args.ref_blocks)] * max(1, args.ref_blocks // pool), rec, dpath) if args.ref_blocks else None
            for n in BLOCKS:
                src, so, sl = batch(streams, n)
                do = torch.arange(n, dtype=i64, device=dev) * rec
                dc = torch.full((n,), rec, dtype=i32, device=dev)
                dst = torch.empty(n * rec + 64, dtype=u8, device=dev)
                out = torch.zeros(n, dtype=i32, device=dev)
                st = torch.cuda.current_stream(dev).cuda_stream
                ts = timed(lambda: amd.DeviceBatch.decompress_safe_dict(src, so, sl, dst, do, dc, out, dict_t))
                oh = out.cpu().numpy()
                decoded = float(oh.astype(np.int64).sum())
                assert decoded == float(n) * rec, "a block of the cell did not decode"
                gbs = sorted(decoded / x / 1e9 for x in ts)
                med = gbs[len(gbs) // 2]
                good, idx = 0, random.Random(n + rec).sample(range(n), min(args.sample, n))
                for i in idx:
                    r, by = ref_decode(streams[i % pool], rec, dbuf, dlen)
                    good += int(oh[i]) == r and dst[i * rec:i * rec + max(r, 0)].cpu().numpy().tobytes() == by
                exact = "n/a"
                if variant is not None:
                    def run_variant():
                        rc = variant.lz4hip_decompress_safe_dict_batch_dev(src.data_ptr(), so.data_ptr(), sl.data_ptr(), dst.data_ptr(), do.data_ptr(),
                                                                          dc.data_ptr(), out.data_ptr(), n, dict_t.data_ptr(), dlen, 0, st)
                        assert rc == 0, rc
                    tv = timed(run_variant)
                    assert float(out.to(i64).sum()) == decoded
                    exact = "%.1f" % (decoded / tv[len(tv) // 2] / 1e9)
                psrc, pso, psl = batch(plain_streams, n)
                tp = timed(lambda: amd.DeviceBatch.decompress_safe(psrc, pso, psl, dst, do, dc, out))
                assert float(out.to(i64).sum()) == decoded
                plain = decoded / tp[len(tp) // 2] / 1e9
                emit("%7d %6d %7d %6.3f %9.1f %16s %8.3f %9s %9.1f %9s %8s %s"
                     % (rec, dlen, n, ratio, med, "%.1f .. %.1f" % (gbs[0], gbs[-1]), ts[len(ts) // 2] * 1e3, exact, plain,
                        "%.2f" % ref_gbs if ref_gbs else "n/a", "%.1fx" % (med / ref_gbs) if ref_gbs else "n/a",
                        "%d/%d bit-exact" % (good, len(idx))))
                del src, psrc, dst
                torch.cuda.empty_cache()
    emit("# GB/s = sum(out_len) / time of the median launch; ratio = compressed / raw bytes of the cell's records with the dictionary;")
    emit("# exact = the developer build whose interior loops leave dictionary matches to the exact path; plain = lz4hip_decompress_safe_batch_dev")
    emit("# on the same records compressed without a dictionary; ref = the reference's LZ4_decompress_safe_usingDict on %d host threads"
         % args.threads)
    emit("# over %d blocks, decoded GB/s (best of three passes)" % args.ref_blocks)
    emit("# %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
