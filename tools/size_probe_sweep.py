#!/usr/bin/env python3
"""tools/size_probe_sweep.py -- the decoded-size query against decoding to scratch, on one MI355X.

The query (lz4hip_decompressed_size_batch_dev) exists to be cheaper than what a caller without it has to do to learn the sizes of a
batch of blocks: decode every block into a scratch slot (lz4hip_decompress_safe_batch_dev) and throw the bytes away.  Both run here
on the same device-resident batch (compressed on the device by lz4hip_compress_fast first; nothing crosses PCIe while timing),
ALTERNATED launch by launch in one session: query, decode, query, decode, ...  The decoder is the one of --baseline-lib (the parent
build's liblz4hip.so) when given, else this build's (its decode kernels disassemble to the parent's instructions).

Batches:  appf64k   SURVEY.md App. F blocks of 64 KiB: 1 / 512 / 2048 / 65536 blocks
          book64k   64 KiB slices of Calgary book1 (tests/golden/calgary/book1.xz, seeded offsets): 2048 / 65536 blocks
          appf4m    App. F blocks of 4 MiB, win 4096: 256 / 2048 blocks
Per point: one warm-up launch of each, then --reps alternated pairs, each launch between its own pair of HIP events on torch's
stream; reported: the median and min .. max of either side in milliseconds, the ratio of the medians, whether the gap exceeds the
spread (query max < decode min), the bytes either side moves by the algorithm (C against C + N), and every out_len of the query
against the decoder's.

  python tools/size_probe_sweep.py [--reps 9] [--baseline-lib PATH] [--out profiles/size_probe_sweep.txt] [--only appf64k,book64k,appf4m]
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
POINTS = {"appf64k": (65536, (1, 512, 2048, 65536)), "book64k": (65536, (2048, 65536)), "appf4m": (4 << 20, (256, 2048))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="appf64k,book64k,appf4m")
    ap.add_argument("--baseline-lib", default=None, help="liblz4hip.so of the parent build: its decoder is the baseline")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 alternated pairs per point"
    import torch
    amd = importlib.import_module("lz4-java_amd")
    dev = torch.device("cuda:0")
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    base = amd.lib()
    if args.baseline_lib:
        base = C.CDLL(os.path.abspath(args.baseline_lib))
        base.lz4hip_decompress_safe_batch_dev.restype = C.c_int
        base.lz4hip_decompress_safe_batch_dev.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_int, C.c_void_p]
        assert not hasattr(base, "lz4hip_decompressed_size_batch_dev"), "--baseline-lib is not the parent build"

    def workload(name, n):
        blk = POINTS[name][0]
        if name == "book64k":
            book = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "calgary", "book1.xz"), "rb").read())
            rng = random.Random(0xB00C1)
            host = bytearray(n * blk)
            for i in range(n):
                o = rng.randrange(len(book) - blk)
                host[i * blk:(i + 1) * blk] = book[o:o + blk]
            src = torch.frombuffer(host, dtype=u8).to(dev)
            del host
        else:
            src = torch.empty(n * blk, dtype=u8, device=dev)
            if name == "appf4m":
                amd.DeviceBatch.gen_blocks(src, blk, blk, n, first_idx=1 << 24, win=4096)
            else:
                amd.DeviceBatch.gen_blocks(src, blk, blk, n)
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
        return blk, comp, co, clen

    def one(run):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# size_probe_sweep: lz4hip_decompressed_size_batch_dev against lz4hip_decompress_safe_batch_dev into scratch slots on %s;"
         % torch.cuda.get_device_name(0))
    emit("# %d alternated pairs per point; decoder: %s" % (args.reps, "the parent build (--baseline-lib)" if args.baseline_lib else "this build"))
    emit("%-8s %7s %9s %19s %9s %19s %7s %7s %10s %10s %s" % ("data", "blocks", "query ms", "min .. max", "decode ms", "min .. max", "ratio",
                                                           "gap", "C MB", "C+N MB", "sizes"))
    lost = []
    for name in args.only.split(","):
        for n in POINTS[name][1]:
            blk, comp, co, clen = workload(name, n)
            do = torch.arange(n, dtype=i64, device=dev) * blk
            dc = torch.full((n,), blk, dtype=i32, device=dev)
            dst = torch.empty(n * blk, dtype=u8, device=dev)
            out_q = torch.zeros(n, dtype=i32, device=dev)
            out_d = torch.zeros(n, dtype=i32, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream

            def query():
                amd.DeviceBatch.decoded_size(comp, co, clen, dc, out_q)

            def decode():
                rc = base.lz4hip_decompress_safe_batch_dev(comp.data_ptr(), co.data_ptr(), clen.data_ptr(), dst.data_ptr(), do.data_ptr(), dc.data_ptr(),
                                                           out_d.data_ptr(), n, 0, st)
                assert rc == 0, rc

            query(); decode()
            torch.cuda.synchronize()
            tq, td = [], []
            for _ in range(args.reps):
                tq.append(one(query))
                td.append(one(decode))
            tq.sort(); td.sort()
            mq, md = tq[len(tq) // 2], td[len(td) // 2]
            same = bool(torch.equal(out_q, out_d)) and bool((out_q == blk).all())
            cbytes = float(clen.to(i64).sum())
            gap = tq[-1] < td[0]
            if not gap:
                lost.append("%s x %d" % (name, n))
            emit("%-8s %7d %9.4f %19s %9.4f %19s %7.3f %7s %10.1f %10.1f %s" % (name, n, mq, "%.4f .. %.4f" % (tq[0], tq[-1]), md,
                                                                             "%.4f .. %.4f" % (td[0], td[-1]), mq / md, "yes" if gap else "NO",
                                                                             cbytes / 1e6, (cbytes + n * blk) / 1e6, "equal" if same else "DIFFER"))
            del comp, dst
            torch.cuda.empty_cache()
    emit("# ms = the median launch between HIP events (launch overhead included on both sides); ratio = query / decode;")
    emit("# gap = the slowest query launch is faster than the fastest decode launch; C = compressed bytes, N = decoded bytes;")
    emit("# sizes = every out_len of the query equals the decoder's and the block size")
    emit("# points where the query is not faster beyond the spread: %s" % (", ".join(lost) if lost else "none"))
    emit("# %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
