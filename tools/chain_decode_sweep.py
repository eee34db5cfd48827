#!/usr/bin/env python3
"""tools/chain_decode_sweep.py -- throughput of the linked-block decoder (LZ4_decompress_safe_continue over chains,
lz4hip_decompress_safe_chain_batch_dev) on one MI355X.

Cells: two kinds of data -- Calgary book1 (tests/golden/calgary/book1.xz, tiled where a chain is longer than the file) and the App. F
synthetic blocks (oracle.gen_block) -- in chains of 1 KiB / 4 KiB / 64 KiB blocks x 16 and 256 blocks per chain x 1 / 256 / 4096 / 65536
chains, device-resident (nothing crosses PCIe while timing).  A pool of distinct chains per cell (at most --pool-mb of raw data) is
compressed on the host by the reference library (LZ4_compress_fast_continue on one stream over the contiguous data: liblz4's prefix
mode) and repeated on the device until the cell's chain count is reached -- every chain has its own copy of its streams and its own
destination.  Cells of more than --max-gb of decoded output are left out (said in their row).

Per cell: one warm-up launch, then --reps timed launches, each between its own pair of HIP events on torch's stream; reported as GB/s
of DECODED output of the median launch (and min .. max):
  chain     decode_chain_kernel: lane groups of 8 walk one chain each, serially
  indep     lz4hip_decompress_safe_batch_dev on the same data compressed as INDEPENDENT blocks of the same size (LZ4_compress_default):
            the ceiling -- what the engine does when nothing links the blocks (and the streams are bigger)
  ref       the reference library's LZ4_decompress_safe_continue on --threads host threads over the first --ref-chains chains (at most --ref-mb of output)
            (tools/chain_decode_refbench.c: pthreads over the dlopen'd library, best of three passes)
and the decoded bytes of a seeded sample of chains against the data the reference compressed.

  python tools/chain_decode_sweep.py [--reps 5] [--out profiles/chain_decode_sweep.txt]
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
BLOCKS = (1024, 4096, 65536)
PER_CHAIN = (16, 256)
CHAINS = (1, 256, 4096, 65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pool-mb", type=int, default=32, help="raw bytes of distinct chains per cell")
    ap.add_argument("--max-gb", type=float, default=4.0, help="cells of more decoded output are left out")
    ap.add_argument("--sample", type=int, default=8, help="chains per cell whose bytes are checked")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the reference's LZ4_decompress_safe_continue")
    ap.add_argument("--ref-chains", type=int, default=4096, help="chains of a cell the reference decodes at most (0 = none)")
    ap.add_argument("--ref-mb", type=int, default=256, help="raw bytes the reference decodes at most per cell (but never fewer chains than threads)")
    ap.add_argument("--data", default="book1,appf")
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
    R.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    R.LZ4_compress_default.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    tmp = tempfile.mkdtemp(prefix="chain_decode_sweep_")
    refbench = os.path.join(tmp, "chain_decode_refbench")
    subprocess.check_call(["gcc", "-O2", "-o", refbench, os.path.join(ROOT, "tools", "chain_decode_refbench.c"), "-lpthread", "-ldl"])

    def raw_chain(kind, k, nbytes):
        """the raw bytes of pool chain k"""
        if kind == "book1":
            o = (k * 104729) % len(book)
            reps = (o + nbytes) // len(book) + 1
            return (book * reps)[o:o + nbytes]
        return O.gen_block(nbytes, 1000 + k)

    def compress_pool(raws, bs):
        """-> (linked streams, independent streams) per block, chain after chain"""
        linked, indep = [], []
        out = C.create_string_buffer(bs + bs // 255 + 64)
        for raw in raws:
            buf = C.create_string_buffer(raw, len(raw))
            st = R.LZ4_createStream()
            for o in range(0, len(raw), bs):
                n = R.LZ4_compress_fast_continue(st, C.addressof(buf) + o, out, bs, len(out), 1)
                assert n > 0
                linked.append(out.raw[:n])
                n = R.LZ4_compress_default(C.addressof(buf) + o, out, bs, len(out))
                assert n > 0
                indep.append(out.raw[:n])
            R.LZ4_freeStream(st)
        return linked, indep

    def ref_rate(streams, bpc, bs):
        sp, lp = os.path.join(tmp, "streams.bin"), os.path.join(tmp, "lens.bin")
        with open(sp, "wb") as fh:
            fh.write(b"".join(streams))
        with open(lp, "wb") as fh:
            fh.write(b"".join(len(s).to_bytes(4, "little") for s in streams))
        c, secs = subprocess.check_output([refbench, ref.path, sp, lp, str(bpc), str(bs), str(args.threads)]).split()
        assert int(c) == (len(streams) // bpc) * bpc * bs, "the reference did not decode every chain"
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

    emit("# chain_decode_sweep: LZ4_decompress_safe_continue over chains on %s, %d timed launches per cell (median, min .. max GB/s of DECODED output)"
         % (torch.cuda.get_device_name(0), args.reps))
    emit("%6s %6s %6s %7s %6s %10s %16s %9s %10s %9s %8s %s" % ("data", "block", "blocks", "chains", "ratio", "chain GB/s", "spread", "ms", "indep GB/s",
                                                              "ref GB/s", "vs ref", "sample"))
    for kind in args.data.split(","):
        for bs in BLOCKS:
            for bpc in PER_CHAIN:
                chain_bytes = bs * bpc
                pc = max(1, min(64, (args.pool_mb << 20) // chain_bytes))
                raws = [raw_chain(kind, k, chain_bytes) for k in range(pc)]
                linked, indep = compress_pool(raws, bs)
                ratio = sum(len(s) for s in linked) / float(chain_bytes * pc)
                ref_cache = {}
                for nch in CHAINS:
                    total = nch * chain_bytes
                    if total > args.max_gb * (1 << 30):
                        emit("%6s %6d %6d %7d %6.3f %10s" % (kind, bs, bpc, nch, ratio, "left out: %.0f GiB of output" % (total / float(1 << 30))))
                        continue
                    n = nch * bpc
                    src, so, sl = batch(linked, n)
                    dc = torch.full((n,), bs, dtype=i32, device=dev)
                    first = (torch.arange(nch + 1, dtype=i64, device=dev) * bpc).to(i32)
                    cdo = torch.arange(nch, dtype=i64, device=dev) * chain_bytes
                    ccap = torch.full((nch,), chain_bytes, dtype=i64, device=dev)
                    dst = torch.empty(total + 64, dtype=u8, device=dev)
                    out = torch.zeros(n, dtype=i32, device=dev)
                    cout = torch.zeros(nch, dtype=i64, device=dev)
                    ts = timed(lambda: amd.DeviceBatch.decompress_safe_chain(src, so, sl, dc, first, dst, cdo, ccap, out, cout))
                    decoded = float(cout.sum().item())
                    assert decoded == float(total), "a chain of the cell did not decode"
                    gbs = sorted(decoded / x / 1e9 for x in ts)
                    med = gbs[len(gbs) // 2]
                    idx = random.Random(nch + bs).sample(range(nch), min(args.sample, nch))
                    good = sum(dst[c * chain_bytes:(c + 1) * chain_bytes].cpu().numpy().tobytes() == raws[c % pc] for c in idx)
                    del src
                    psrc, pso, psl = batch(indep, n)
                    do = torch.arange(n, dtype=i64, device=dev) * bs
                    tp = timed(lambda: amd.DeviceBatch.decompress_safe(psrc, pso, psl, dst, do, dc, out))
                    assert float(out.to(i64).sum().item()) == decoded
                    plain = decoded / tp[len(tp) // 2] / 1e9
                    rch = min(nch, args.ref_chains, max(args.threads, (args.ref_mb << 20) // chain_bytes))
                    if rch and rch not in ref_cache:
                        ref_cache[rch] = ref_rate((linked * ((rch + pc - 1) // pc))[:rch * bpc], bpc, bs)
                    ref_gbs = ref_cache.get(rch)
                    emit("%6s %6d %6d %7d %6.3f %10.2f %16s %9.3f %10.1f %9s %8s %s"
                         % (kind, bs, bpc, nch, ratio, med, "%.2f .. %.2f" % (gbs[0], gbs[-1]), ts[len(ts) // 2] * 1e3, plain,
                            "%.2f" % ref_gbs if ref_gbs else "n/a", "%.2fx" % (med / ref_gbs) if ref_gbs else "n/a",
                            "%d/%d bit-exact" % (good, len(idx))))
                    del psrc, dst
                    torch.cuda.empty_cache()
    emit("# GB/s = decoded bytes / time of the median launch; ratio = linked compressed / raw bytes of the cell's chains; indep =")
    emit("# lz4hip_decompress_safe_batch_dev on the same data compressed as independent blocks; ref = the reference's")
    emit("# LZ4_decompress_safe_continue on %d host threads over up to %d chains, decoded GB/s (best of three passes): with fewer chains than" % (args.threads, args.ref_chains))
    emit("# threads only that many threads have work")
    emit("# %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
