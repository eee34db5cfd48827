#!/usr/bin/env python3
"""tools/dstream_inorder_sweep.py -- what the in-order twin of the stream decoder costs (lz4hip_decompress_safe_stream_inorder_batch,
decode_stream_inorder_kernel) beside this build's decode_stream_kernel on one MI355X.

Both entry points take host pointers, so wall time is staging; what is compared is KERNEL time.  Every cell runs in a child process of
its own under `rocprofv3 --kernel-trace --stats` (nothing else is collected in that run), and the kernels' times are read from the
child's kernel trace.  A cell is N streams of 16 x 4 KiB blocks, written by the reference library's LZ4_compress_fast_continue (one
LZ4_stream_t per stream over contiguous data), decoded in ONE call each by
  stream    decode_stream_kernel, the blocks back to back from a fresh state (tools/dstream_sweep.py's layout a)
  (i)       decode_stream_inorder_kernel on the same, knob 0: no slot overlaps, so the same decode_block instances run
  (ii)      the same, knob 1: every block through the in-order tier -- the price of the tier itself
  (iii)     knob 0, liblz4's minimal ring of 65536 + 14 + 4096 bytes, entered behind ENTER bytes of (never read) history so that the
            fifth block wraps to 0: four blocks on the rolling prefix, then twelve whose slots overlap the last 65535 bytes of what the
            ring held -- those take the in-order tier; beside it decode_stream_kernel on the same ring (its bytes are unspecified there,
            its time is not)
on Calgary book1 (tests/golden/calgary/book1.xz) and the App. F synthetic blocks (oracle.gen_block); a pool of 512 distinct streams is
tiled to the cell's stream count.  The child checks that every call gives the same results and, on a sample, the writer's bytes.

  python tools/dstream_inorder_sweep.py [--streams 65536,4096] [--data appf,book1] [--out profiles/dstream_inorder_sweep.txt]
"""
import argparse
import ctypes as C
import importlib
import lzma
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dstream_sweep import trace_ns   # noqa: E402

BLOCK, BLOCKS = 4096, 16
RING = 65536 + 14 + BLOCK
ENTER = RING - 4 * BLOCK - 100


def ring_places():
    """-> (window offset of every block, how many of them have a slot that overlaps the history they can reach): the walk's own test"""
    pos, p = [], ENTER
    pe, pl, ee, el, over = ENTER, ENTER, 0, 0, 0
    for _ in range(BLOCKS):
        if p + BLOCK > RING:
            p = 0
        grows = pl != 0 and pe == p
        if pl != 0 and not grows:
            ee, el = pe, pl
        reach = min(el, 65535 - (min(pl, 65535) if grows else 0))
        over += 1 if (el and reach and p < ee and p + BLOCK > ee - reach) else 0
        pe, pl = (pe + BLOCK, pl + BLOCK) if grows else (p + BLOCK, BLOCK)
        pos.append(p); p += BLOCK
    return pos, over


def worker(kind, n):
    """one cell, no timing of its own; prints `cell ok <decoded bytes> <blocks of (iii) in order>`"""
    import numpy as np
    amd = importlib.import_module("lz4-java_amd")
    from oracle import oracle as O
    L = C.CDLL(O.ref().path)
    L.LZ4_createStream.restype = C.c_void_p
    L.LZ4_freeStream.argtypes = [C.c_void_p]
    L.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    book = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "calgary", "book1.xz"), "rb").read())
    stride = BLOCK * BLOCKS
    pool = min(512, n)

    def raw(k):
        if kind == "book1":
            o = (k * 104729) % (len(book) - stride)
            return book[o:o + stride]
        return O.gen_block(stride, 1000 + k)
    raws, comp, lens = [], bytearray(), []
    for k in range(pool):
        r = raw(k)
        raws.append(r)
        buf = C.create_string_buffer(r, stride)
        st = L.LZ4_createStream()
        for i in range(BLOCKS):
            dst = C.create_string_buffer(BLOCK + BLOCK // 255 + 32)
            m = L.LZ4_compress_fast_continue(st, C.addressof(buf) + i * BLOCK, dst, BLOCK, len(dst), 1)
            assert m > 0
            comp += dst.raw[:m]; lens.append(m)
        L.LZ4_freeStream(st)
    reps = (n + pool - 1) // pool
    src = np.tile(np.frombuffer(bytes(comp), dtype=np.uint8), reps)
    src_len = np.tile(np.array(lens, dtype=np.int32), reps)[:n * BLOCKS]
    src_off = np.concatenate([[0], np.cumsum(src_len.astype(np.uint64))[:-1]]).astype(np.uint64)
    first = np.arange(n + 1, dtype=np.uint32) * np.uint32(BLOCKS)
    cap = np.full(n * BLOCKS, BLOCK, np.int32)
    sample = list(range(0, n, max(1, n // 64)))
    fresh = [(0, 0, 0, 0)] * n
    f = amd.LZ4HIPBatch.decompressSafeStream
    # back to back: the existing call, then the twin with the knob at 0 and at 1
    win_off = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    win_len = np.full(n, stride, np.uint64)
    dst_off = (np.arange(n * BLOCKS, dtype=np.uint64) * np.uint64(BLOCK))
    dst = np.zeros(n * stride, np.uint8)
    for in_order, every in ((False, 0), (True, 0), (True, 1)) * 2:   # (twice: the first round also pays for the first touch of every buffer)
        dst[:] = 0
        amd.set_option("dstream_inorder", every)
        out, state = f(fresh, src, src_off, src_len, first, dst, dst_off, cap, win_off, win_len, inOrder=in_order)
        assert (out == BLOCK).all() and all(s[1] == stride for s in state)
        for c in sample:
            assert dst[c * stride:(c + 1) * stride].tobytes() == raws[c % pool], "back to back: the bytes"
    amd.set_option("dstream_inorder", 0)
    del dst
    # the minimal ring: the twin, then the existing call
    pos, over = ring_places()
    assert pos[4] == 0 and over == 12
    ring = np.zeros(n * RING, np.uint8)
    win_off = np.arange(n, dtype=np.uint64) * np.uint64(RING)
    win_len = np.full(n, RING, np.uint64)
    dst_off = (win_off[:, None] + np.array(pos, dtype=np.uint64)[None, :]).reshape(-1)
    entered = [(int(w) + ENTER, ENTER, 0, 0) for w in win_off]
    for in_order in (True, False):
        out, state = f(entered, src, src_off, src_len, first, ring, dst_off, cap, win_off, win_len, inOrder=in_order)
        assert (out == BLOCK).all() and all(s[1] == 12 * BLOCK for s in state)
        if in_order:
            for c in sample:
                got = b"".join(ring[c * RING + q:c * RING + q + BLOCK].tobytes() for q in pos)
                assert got == raws[c % pool], "the minimal ring: the bytes"
    print("cell ok %d %d" % (n * stride, over), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="65536,4096")
    ap.add_argument("--data", default="appf,book1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--work", default=None, help="directory for the profiler's output of every cell (default: beside --out, else the current directory)")
    ap.add_argument("--cell-timeout", type=int, default=420)
    ap.add_argument("--worker", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], int(args.worker[1]))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# dstream_inorder_sweep: kernel time of decode_stream_inorder_kernel beside this build's decode_stream_kernel (N streams x 16 blocks of 4 KiB in")
    emit("# ONE call; back to back, and a minimal ring of %d bytes entered at %d: %d of 16 blocks in order); rocprofv3 --kernel-trace --stats, one run per cell"
         % (RING, ENTER, ring_places()[1]))
    emit("%6s %8s %10s %10s %10s %10s %10s %9s %9s %9s" % ("data", "streams", "stream ms", "(i) ms", "(ii) ms", "(iii) ms", "ring ms", "(i)/strm", "(ii)/strm", "(iii)/ring"))
    work = args.work or (os.path.dirname(os.path.abspath(args.out)) if args.out else os.getcwd())
    os.makedirs(work, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="dstream_inorder_sweep_", dir=work)
    stop = False
    for kind in args.data.split(","):
        for n in (int(v) for v in args.streams.split(",")):
            d = os.path.join(tmp, "%s_%d" % (kind, n))
            # (timeout -k: the profiler AND the worker behind it end with the time limit; start_new_session + killpg below: nothing of the
            # cell outlives it, whatever ended it)
            cmd = ["timeout", "-k", "10", str(args.cell_timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--worker", kind, str(n)]
            p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
            try:
                so, se = p.communicate(timeout=args.cell_timeout + 30)
                status, tail = p.returncode, (se or so)[-300:].replace("\n", " | ")
                good = status == 0 and "cell ok" in so
            except subprocess.TimeoutExpired:
                status, tail, good = 124, "time limit", False
            finally:
                try:
                    os.killpg(p.pid, signal.SIGKILL)   # (the group is gone after a clean end: nothing to do then)
                except (ProcessLookupError, PermissionError):
                    pass
                if p.poll() is None:
                    p.wait()
            if not good:   # (whatever ended it: nothing more is started on the device after a run that failed)
                emit("# %s %d: the cell's run failed (status %d): %s" % (kind, n, status, tail))
                emit("# stopping here")
                stop = True
                break
            st, io = trace_ns(d, "decode_stream_kernel"), trace_ns(d, "decode_stream_inorder_kernel")
            # (the host path cuts a call into chunks, each a launch: la per back-to-back call, ld per ring call; the back-to-back calls
            # run in two rounds, so the existing kernel ran 2 la + ld launches and the twin 4 la + ld; the SECOND round is reported)
            la = (len(io) - len(st)) // 2
            ld = len(st) - 2 * la
            if la < 1 or ld < 1 or (len(io) - len(st)) % 2:
                emit("# %s %d: no usable kernel rows (%d stream launches, %d in-order launches)" % (kind, n, len(st), len(io)))
                continue
            s_ns, r_ns = sum(st[la:2 * la]), sum(st[2 * la:])
            i_ns, ii_ns, iii_ns = sum(io[2 * la:3 * la]), sum(io[3 * la:4 * la]), sum(io[4 * la:])
            first_round = "%.3f / %.3f" % (sum(io[:la]) / sum(st[:la]), sum(io[la:2 * la]) / sum(st[:la]))
            emit("%6s %8d %10.3f %10.3f %10.3f %10.3f %10.3f %9.3f %9.3f %9.3f"
                 % (kind, n, s_ns / 1e6, i_ns / 1e6, ii_ns / 1e6, iii_ns / 1e6, r_ns / 1e6, i_ns / s_ns, ii_ns / s_ns, iii_ns / r_ns))
            emit("#   (first round, where the existing kernel's call is the first to touch the buffers: (i) / (ii) = %s of it)" % first_round)
            shutil.rmtree(d, ignore_errors=True)
        if stop:
            break
    emit("# ms = total kernel time of the call's launches (the host path cuts a call into chunks of 64 MiB of compressed bytes or 512 MiB of device")
    emit("# image, each a launch).  The three back-to-back calls run twice in turn and the second round is what the columns show.")
    emit("# stream: decode_stream_kernel, back to back; (i) / (ii): the twin on the same, knob 0 / 1; (iii): the twin on the")
    emit("# minimal ring, knob 0 (12 of 16 blocks decoded in order); ring: decode_stream_kernel on that ring.  decode_stream_kernel is")
    emit("# instruction-identical to the parent's (profiles/dstream_inorder_kernel_diff.txt).  %s" % time.strftime("%Y-%m-%d %H:%M:%S"))
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
