#!/usr/bin/env python3
"""tools/chain_compress_sweep.py -- throughput of the linked-block compressor (LZ4_compress_fast_continue over chains,
lz4hip_compress_fast_chain_batch_dev) on one MI355X.

Cells: two kinds of data -- Calgary book1 (tests/golden/calgary/book1.xz, tiled where a chain is longer than the file) and the App. F
synthetic blocks (oracle.gen_block) -- in 65536 / 4096 / 1 chains of 16 x 4 KiB blocks and 65536 chains of 64 x 1 KiB blocks, each
without a prefix and behind 64 KiB of history, device-resident (nothing crosses PCIe while timing).  A pool of distinct chains per cell
(at most --pool-mb of raw data, history included) is repeated on the device until the cell's chain count is reached -- every chain
has its own copy of its history and source and its own slots of the bound.

Per cell: one warm-up launch, then --reps timed launches, each between its own pair of HIP events on torch's stream; reported as GB/s
of SOURCE consumed in the median launch (and min .. max):
  chain     compress_fast_chain_cu_kernel: one wavefront walks one chain, serially, its table kept in LDS from block to block
  indep     lz4hip_compress_fast_batch_dev on the same blocks taken as INDEPENDENT blocks: what the engine does when nothing links them
  sizes     compressed bytes / source bytes of the two
  ref       the reference library's LZ4_compress_fast_continue on --threads host threads, chains dealt to the threads, over the first
            --ref-chains chains (at most --ref-mb of source): tools/chain_compress_refbench.c, best of three passes
and the bytes of a seeded sample of chains against the reference library's output for the same chain.

  python tools/chain_compress_sweep.py [--reps 5] [--out profiles/chain_compress_sweep.txt]
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
CELLS = ((65536, 16, 4096), (4096, 16, 4096), (1, 16, 4096), (65536, 64, 1024))   # chains, blocks per chain, block bytes
PREFIXES = (0, 65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pool-mb", type=int, default=32, help="raw bytes of distinct chains per cell")
    ap.add_argument("--sample", type=int, default=4, help="chains per cell whose bytes are checked against the reference")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the reference's LZ4_compress_fast_continue")
    ap.add_argument("--ref-chains", type=int, default=4096, help="chains of a cell the reference compresses at most (0 = none)")
    ap.add_argument("--ref-mb", type=int, default=256, help="source bytes the reference compresses at most per cell (never fewer chains than threads)")
    ap.add_argument("--data", default="appf,book1")
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
    R.LZ4_loadDict.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    R.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    tmp = tempfile.mkdtemp(prefix="chain_compress_sweep_")
    refbench = os.path.join(tmp, "chain_compress_refbench")
    subprocess.check_call(["gcc", "-O2", "-o", refbench, os.path.join(ROOT, "tools", "chain_compress_refbench.c"), "-lpthread", "-ldl"])

    def raw_chain(kind, k, nbytes):
        """history and source of pool chain k, back to back"""
        if kind == "book1":
            o = (k * 104729) % len(book)
            reps = (o + nbytes) // len(book) + 1
            return (book * reps)[o:o + nbytes]
        return O.gen_block(nbytes, 1000 + k)

    def ref_chain(raw, P, bpc, bs):
        buf = C.create_string_buffer(raw, len(raw))
        st = R.LZ4_createStream()
        if P:
            R.LZ4_loadDict(st, buf, P)
        out = C.create_string_buffer(bs + bs // 255 + 64)
        res = []
        for i in range(bpc):
            n = R.LZ4_compress_fast_continue(st, C.addressof(buf) + P + i * bs, out, bs, bs + bs // 255 + 16, 1)
            assert n > 0
            res.append(out.raw[:n])
        R.LZ4_freeStream(st)
        return res

    def ref_rate(raws, P, bpc, bs):
        dp = os.path.join(tmp, "data.bin")
        with open(dp, "wb") as fh:
            fh.write(b"".join(raws))
        c, p, secs = subprocess.check_output([refbench, ref.path, dp, str(P), str(bpc), str(bs), str(args.threads)]).split()
        assert int(c) == len(raws) * bpc * bs, "the reference did not compress every chain"
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

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# chain_compress_sweep: LZ4_compress_fast_continue over chains on %s, %d timed launches per cell (median, min .. max GB/s of SOURCE)"
         % (torch.cuda.get_device_name(0), args.reps))
    emit("%6s %6s %6s %7s %7s %10s %16s %9s %10s %11s %11s %9s %8s %s" % ("data", "block", "blocks", "chains", "prefix", "chain GB/s", "spread", "ms", "indep GB/s",
                                                                        "chain size", "indep size", "ref GB/s", "vs ref", "sample"))
    for kind in args.data.split(","):
        for nch, bpc, bs in CELLS:
            for P in PREFIXES:
                chain_bytes = bs * bpc
                stride = P + chain_bytes
                pc = max(1, min(512, nch, (args.pool_mb << 20) // stride))
                raws = [raw_chain(kind, k, stride) for k in range(pc)]
                reps = (nch + pc - 1) // pc
                src = torch.from_numpy(np.frombuffer(b"".join(raws), dtype=np.uint8).copy()).to(dev).repeat(reps)
                src = torch.cat([src, torch.zeros(64, dtype=u8, device=dev)])
                n = nch * bpc
                cap = bs + bs // 255 + 16
                cso = torch.arange(nch, dtype=i64, device=dev) * stride + P
                pre = torch.full((nch,), P, dtype=i32, device=dev)
                sl = torch.full((n,), bs, dtype=i32, device=dev)
                first = (torch.arange(nch + 1, dtype=i64, device=dev) * bpc).to(i32)
                do = torch.arange(n, dtype=i64, device=dev) * cap
                dc = torch.full((n,), cap, dtype=i32, device=dev)
                dst = torch.empty(n * cap + 64, dtype=u8, device=dev)
                out = torch.zeros(n, dtype=i32, device=dev)
                cons = torch.zeros(nch, dtype=i64, device=dev)
                ts = timed(lambda: amd.DeviceBatch.compress_fast_chain(src, cso, sl, first, dst, do, dc, out, cons, pre if P else None))
                total = float(cons.sum().item())
                assert total == float(nch * chain_bytes), "a chain of the cell stopped"
                gbs = sorted(total / x / 1e9 for x in ts)
                med = gbs[len(gbs) // 2]
                csize = float(out.to(i64).sum().item())
                idx = random.Random(nch + bs + P).sample(range(nch), min(args.sample, nch))
                good = 0
                for c in idx:
                    want = ref_chain(raws[c % pc], P, bpc, bs)
                    o_c = out[c * bpc:(c + 1) * bpc].cpu().tolist()
                    got = [dst[(c * bpc + i) * cap:(c * bpc + i) * cap + o_c[i]].cpu().numpy().tobytes() for i in range(bpc)]
                    good += got == want
                # the same blocks as independent blocks
                so = (cso[:, None] + (torch.arange(bpc, dtype=i64, device=dev) * bs)[None, :]).reshape(-1).contiguous()
                tp = timed(lambda: amd.DeviceBatch.compress_fast(src, so, sl, dst, do, dc, out))
                isize = float(out.to(i64).sum().item())
                plain = total / tp[len(tp) // 2] / 1e9
                rch = min(nch, args.ref_chains, max(args.threads, (args.ref_mb << 20) // stride))
                ref_gbs = ref_rate((raws * ((rch + pc - 1) // pc))[:rch], P, bpc, bs) if rch else None
                emit("%6s %6d %6d %7d %7d %10.2f %16s %9.3f %10.1f %11.4f %11.4f %9s %8s %s"
                     % (kind, bs, bpc, nch, P, med, "%.2f .. %.2f" % (gbs[0], gbs[-1]), ts[len(ts) // 2] * 1e3, plain, csize / total, isize / total,
                        "%.2f" % ref_gbs if ref_gbs else "n/a", "%.2fx" % (med / ref_gbs) if ref_gbs else "n/a", "%d/%d bit-exact" % (good, len(idx))))
                del src, dst
                torch.cuda.empty_cache()
    emit("# GB/s = source bytes / time of the median launch; chain size / indep size = compressed bytes / source bytes of the linked chains and of")
    emit("# the same blocks compressed independently (lz4hip_compress_fast_batch_dev); ref = the reference's LZ4_compress_fast_continue on %d host" % args.threads)
    emit("# threads over up to %d chains, source GB/s (best of three passes): with fewer chains than threads only that many threads have work" % args.ref_chains)
    emit("# %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
