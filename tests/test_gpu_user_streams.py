"""The stream contract of include/lz4hip.h on the GPU -- work is "enqueued on `stream`", the call "returns without synchronising" --
for every device entry point of tests/userstream_common.py's table, on streams of the caller's:

  B1  every entry on a side stream behind a filler kernel: the call returns while the filler still runs (or, where the header says
      that it waits for its stream, after it), reads what the stream brought in behind the filler and has written everything when
      the stream reaches the snapshot;
  B2  pairs of entries that take the same kind of library-owned scratch, on two streams at once, from one host thread and from two;
  B3  one streaming-xxhash handle fed from two streams in turn;
  B4  the route word of a routed decode launch, reused by a launch of another stream while the first launch still runs;
  B5  the second and later calls of a process, with and without a synchronisation between them.

Expected values are the reference's (userstream_common.py).  Figures the tests measure (the filler's length, every entry's host-side
call time) go to the file the environment variable LZ4HIP_USERSTREAM_NOTES names, if it is set."""
import os
import threading
import time

import numpy as np
import pytest

import userstream_common as U

pytestmark = pytest.mark.gpu
FILLER_MS = 50.0
ROUNDS = 20


def note(line):
    path = os.environ.get("LZ4HIP_USERSTREAM_NOTES")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def dev(amd):
    import torch
    amd.lib()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def filler(dev):
    """cycles of torch.cuda._sleep that take about FILLER_MS: a fixed count timed with two events, then scaled"""
    import torch
    probe = 1_000_000
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); torch.cuda._sleep(probe); b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 0.2, ("the sleep kernel does not sleep", ms)
    cycles = int(probe * FILLER_MS / ms)
    a.record(); torch.cuda._sleep(cycles); b.record()
    torch.cuda.synchronize()
    got = a.elapsed_time(b)
    note("filler: torch.cuda._sleep(%d) took %.2f ms -> %d cycles for %.0f ms, measured %.2f ms" % (probe, ms, cycles, FILLER_MS, got))
    assert 0.5 * FILLER_MS <= got <= 2.0 * FILLER_MS, got
    return cycles, got


_TORCH = {"int32": "int32", "int64": "int64", "uint32": "int32", "uint64": "int64"}


class Run:
    """one case on the device: the source buffer, the arrays the entry reads, the destination, the arrays it writes, and the real input
    Y and the decoy X with their arrays beside them"""

    def __init__(self, amd, dev, case):
        import torch
        self.amd, self.dev, self.case, self.torch = amd, dev, case, torch
        up = lambda by: torch.frombuffer(bytearray(by or b"\0"), dtype=torch.uint8).to(dev)
        arr = lambda dtype, v: torch.from_numpy(np.asarray(v if len(v) else [0]).astype(dtype)).to(dev)
        self.y, self.x = up(case.src_y), up(case.src_x)
        self.real = {k: arr(d, v) for k, (d, v, _) in case.ins.items()}
        self.decoy = {k: arr(d, v) for k, (d, _, v) in case.ins.items()}
        self.t = {"src": torch.empty_like(self.y), "dst": torch.empty(max(case.dst_len, 1), dtype=torch.uint8, device=dev)}
        for k, v in self.real.items():
            self.t[k] = torch.empty_like(v)
        self.outs = {k: torch.empty(max(len(want), 1), dtype=getattr(torch, _TORCH[d]), device=dev) for k, (d, want, _) in case.outs.items()}
        self.t.update(self.outs)
        if case.setup:
            self.t.update(case.setup(amd, torch, dev))

    def close(self):
        if self.case.teardown:
            self.case.teardown(self.t)

    def arm(self):
        """the decoy and its arrays in, the destination and the result arrays blank (on the current stream)"""
        self.t["src"].copy_(self.x)
        for k, v in self.decoy.items():
            self.t[k].copy_(v)
        self.blank()

    def blank(self):
        self.t["dst"].fill_(U.FILL)
        for v in self.outs.values():
            v.fill_(U.SENTINEL)

    def bring(self):
        """the real input and its arrays over the decoys (on the current stream)"""
        self.t["src"].copy_(self.y)
        for k, v in self.real.items():
            self.t[k].copy_(v)

    def call(self):
        self.case.call(self.amd, self.t)

    def snapshot(self):
        """copies of the destination and of every result array, taken on the current stream"""
        snap = {"dst": self.t["dst"].clone()}
        snap.update({k: v.clone() for k, v in self.outs.items()})
        return snap

    def problems(self, snap=None):
        """(the stream is done) what the snapshot -- or the tensors themselves -- hold against the reference"""
        snap = snap or dict(self.outs, dst=self.t["dst"])
        got = {k: snap[k].cpu().tolist()[:len(self.case.outs[k][1])] for k in self.outs}
        if self.case.after:
            got.update(self.case.after(self.amd, self.t))
        return U.check(self.case, snap["dst"].cpu().numpy().tobytes()[:self.case.dst_len], got)


@pytest.fixture(scope="module")
def case_of(ref, O, corpus):
    return lambda fn: U.case_of(fn, ref, O, corpus)


# ---- B1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", sorted(U.TABLE))
def test_stream_order_and_return_without_synchronising(amd, dev, filler, case_of, fn):
    """On a side stream S, with nothing synchronised in between: a filler kernel, an event E behind it, the real input Y and its arrays
    copied over the decoys (and the destination blanked once more), the call, snapshots of the destination and the result arrays.
    Right after the call E is still pending -- the call did not wait for S -- unless the header says it does; after S.synchronize()
    alone the snapshots hold the reference's result for Y, every guard is intact and nothing is the decoy's result.  A kernel, a memset
    or a copy that the library puts on another stream runs while S sleeps: it reads the decoy or zero lengths, or its output is blanked
    and missing from the snapshot.  Directly in front of the call, the same entry runs once on the decoy with buffers of its own (the
    PRIMER): it takes the stream-ordered scratch that the call takes next and leaves it dirty, so that a memset of the call's which runs
    early, on another stream, is undone before the call's kernels start.  (A first, unmeasured call of both grows the memory pool and
    builds a dictionary's images; a second one is timed on the host without a filler.)"""
    import torch
    cycles, filler_ms = filler
    e = U.TABLE[fn]
    run, primer = Run(amd, dev, case_of(fn)), Run(amd, dev, case_of(fn))
    S = torch.cuda.Stream()
    try:
        with torch.cuda.stream(S):
            primer.bring(); primer.t["src"].copy_(primer.x); primer.blank(); primer.call()
            run.arm(); run.bring(); run.call()
            S.synchronize()
            assert run.problems() == [], (fn, "the warm-up call")
            run.arm(); run.bring()
            S.synchronize()
            t0 = time.perf_counter()
            run.call()
            host_ms = (time.perf_counter() - t0) * 1e3
            S.synchronize()
            note("B1 %s: host-side call time %.3f ms (syncs=%s)" % (fn, host_ms, e.syncs))
            assert run.problems() == [], (fn, "the timed call")
            if not e.syncs:
                assert 10 * host_ms <= filler_ms, (fn, "the filler is not ten times the call's host time", host_ms, filler_ms)
            run.arm()
            torch.cuda.synchronize()
            torch.cuda._sleep(cycles)
            E = torch.cuda.Event()
            E.record(S)
            run.bring()
            run.t["dst"].fill_(U.FILL)
            primer.call()
            run.call()
            early = E.query()
            snap = run.snapshot()
        if e.syncs:
            assert early, (fn, "the header says that the call waits for its stream; it returned while the filler ran")
        else:
            assert not early, (fn, "the call waited for its stream: the filler of %.0f ms was over when it returned (host time %.3f ms)" % (filler_ms, host_ms))
        S.synchronize()
        bad = run.problems(snap)
        assert bad == [], (fn, len(bad), bad[:4])
    finally:
        torch.cuda.synchronize()
        run.close()
        primer.close()


# ---- B2 --------------------------------------------------------------------------------------------------------------------------------
def prepared(amd, dev, case, rounds=ROUNDS):
    """one Run per round, each with its own device buffers, the real input in place"""
    runs = [Run(amd, dev, case) for _ in range(rounds)]
    for r in runs:
        r.bring(); r.blank()
    return runs


def run_sides(sides, threads, before=None, after=None):
    """sides = [(stream, [Run per round])]: every round's calls enqueued side by side from one host thread, alternating, or each side's
    rounds from a thread of its own; nothing waits for the device in between.  before(side, round) / after(side, round) run on the
    side's stream around its call"""
    import torch
    rounds = len(sides[0][1])
    errors = []

    def one(k, r):
        S, runs = sides[k]
        with torch.cuda.stream(S):
            if before:
                before(k, r)
            runs[r].call()
            if after:
                after(k, r)

    def side(k):
        try:
            for r in range(rounds):
                one(k, r)
        except Exception as ex:          # (a thread's failure is the test's)
            errors.append((k, repr(ex)))
    if threads:
        ts = [threading.Thread(target=side, args=(k,)) for k in range(len(sides))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    else:
        for r in range(rounds):
            for k in range(len(sides)):
                one(k, r)
    for S, _ in sides:
        S.synchronize()
    assert not errors, errors
    bad = [(k, r, p[:3]) for k, (_, runs) in enumerate(sides) for r, run in enumerate(runs) for p in [run.problems()] if p]
    assert not bad, (len(bad), bad[:4])


def both_ways(amd, dev, cases, **kw):
    import torch
    for threads in (False, True):
        sides = [(torch.cuda.Stream(), prepared(amd, dev, c)) for c in cases]
        try:
            torch.cuda.synchronize()
            run_sides(sides, threads, **kw)
        finally:
            torch.cuda.synchronize()
            for _, runs in sides:
                for r in runs:
                    r.close()


PAIRS = {
    "fast x fast": ("lz4hip_compress_fast_batch_dev", "lz4hip_compress_fast_batch_dev"),
    "fast x accel x destSize": ("lz4hip_compress_fast_batch_dev", "lz4hip_compress_fast_accel_batch_dev", "lz4hip_compress_dest_size_batch_dev"),
    "chain decode x chain compress": ("lz4hip_decompress_safe_chain_batch_dev", "lz4hip_compress_fast_chain_batch_dev"),
    "containers": ("lz4hip_container_blocks_dev", "lz4hip_container_decode_dev"),
}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_two_streams_at_once(amd, dev, case_of, pair):
    """entries that take the same kind of library-owned scratch (queue words, routed-block lists, mail rings: stream-ordered
    allocations) on a stream each, ROUNDS rounds without a host synchronisation, every round with buffers of its own; all results
    against the reference at the end.  From one host thread, alternating, then from a thread per stream"""
    both_ways(amd, dev, [case_of(fn) for fn in PAIRS[pair]])


def test_two_streams_dictionary_handle(amd, dev, case_of):
    """fast and HC dictionary compress on ONE handle (its two images), and the dictionary decoder, on a stream each"""
    dic = amd.LZ4Dictionary(U.F.dict_of(U.DICT_LEN))
    try:
        fns = ("lz4hip_compress_fast_dict_batch_dev", "lz4hip_compress_hc_dict_batch_dev_ws", "lz4hip_decompress_safe_dict_batch_dev")
        cases = [case_of(fn)._replace(setup=None if fn.startswith("lz4hip_compress") else case_of(fn).setup, teardown=None) for fn in fns]
        import torch
        for threads in (False, True):
            sides = []
            for c in cases:
                runs = prepared(amd, dev, c)
                if c.setup is None:
                    for r in runs:
                        r.t["dic"] = dic
                sides.append((torch.cuda.Stream(), runs))
            # (the handle's first compress of each kind builds its image and waits for its stream once: made here, before the rounds)
            for S, runs in sides[:2]:
                with torch.cuda.stream(S):
                    runs[0].call()
                S.synchronize()
                runs[0].blank()
            torch.cuda.synchronize()
            run_sides(sides, threads)
    finally:
        import torch
        torch.cuda.synchronize()
        dic.close()


def test_two_streams_routed_decoders(amd, dev, ref, O, corpus):
    """the safe decoder on text and the fast decoder on App. F blocks, both routed on the device (16 CU + 1 blocks: each launch takes a
    route word of the device's ring) -- and that they were: last_decode_route holds the sampler's figures"""
    import torch
    n = 16 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    cases = [U.routed_case(ref, O, corpus, "text", False, n), U.routed_case(ref, O, corpus, "appf", True, n)]
    for c in cases:              # each alone: the launch is routed, the sampler found streams to read
        run = Run(amd, dev, c)
        run.bring(); run.blank(); run.call()
        torch.cuda.synchronize()
        route = amd.last_decode_route()
        lens = c.ins["src_len"][1]
        assert route[3] == sum(lens[i * (n // 64)] for i in range(64)) // 64 and route[5] > 0 and route[2] > 0, ("the launch was not routed", route)
        assert run.problems() == []
    both_ways(amd, dev, cases)


def test_hc_sync_waits_for_its_own_stream_only(amd, dev, filler, case_of, ref, O, corpus):
    """lz4hip_compress_hc_batch_dev synchronises `stream` -- that stream: while a safe decode on another stream sits behind a filler,
    every HC call returns with the filler still running.  (The HC batch holds the blocks of up to 4 KiB only: each call waits for the
    kernels of the one before it on its own stream, and those must not take as long as a filler does.)"""
    import torch
    cycles, filler_ms = filler
    cases = [case_of("lz4hip_decompress_safe_batch_dev"), U.compress_hc_sync_small_case(ref, O, corpus)]     # (each round: the decode side first)
    for threads in (False, True):
        sides = [(torch.cuda.Stream(), prepared(amd, dev, c)) for c in cases]
        events, early = {}, []

        def before(k, r):
            if k == 0:
                torch.cuda._sleep(cycles)
                events[r] = torch.cuda.Event()
                events[r].record()

        def after(k, r):
            # (one thread: round r's filler is in place, behind r others, when the HC call is made; two threads: the decode side may
            # not have reached round r yet -- then there is nothing to ask)
            ev = events.get(r) if k == 1 else None
            if ev is not None and ev.query():
                early.append(r)
        try:
            torch.cuda.synchronize()
            run_sides(sides, threads, before=before, after=after)
            assert not early, ("the HC call waited for the other stream's filler in rounds", early)
            assert threads or len(events) == ROUNDS
        finally:
            torch.cuda.synchronize()


# ---- B3 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (32, 64))
def test_one_xxh_stream_handle_fed_from_two_streams(amd, dev, ref, filler, bits):
    """300000 random bytes in pieces, piece k through update_device on stream k % 2, the odd pieces' stream behind a filler; no host
    synchronisation until getValue().  The library orders the updates of one handle across streams (an event per handle): the digest
    is the one-shot hash of the whole.  Again after reset()"""
    import random
    import torch
    cycles, _ = filler
    seed = 0x9747b28c
    data = random.Random(23).randbytes(300000)
    d = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    want = (ref.xxh32 if bits == 32 else ref.xxh64)(data, seed)
    h = (amd.StreamingXXHash32 if bits == 32 else amd.StreamingXXHash64)(seed)
    S = (torch.cuda.Stream(), torch.cuda.Stream())
    try:
        torch.cuda.synchronize()
        for trial in range(2):
            pieces = U.xxh_pieces(len(data), 31 + trial)
            assert len(pieces) > 20 and sum(n for _, n in pieces) == len(data)
            with torch.cuda.stream(S[1]):
                torch.cuda._sleep(cycles)
            for k, (o, n) in enumerate(pieces):
                h.update_device(d.data_ptr() + o, n, stream=S[k % 2].cuda_stream)
            assert h.getValue() == want, (bits, trial)
            h.reset()
    finally:
        torch.cuda.synchronize()
        h.close()


# ---- B4 --------------------------------------------------------------------------------------------------------------------------------
V_BLOCK, K_BLOCKS, GUARD = 16384, 40960, U.GUARD


class Routed:
    """a routed decode launch with its own output: the source blocks back to back in `want`, the streams in `comp`"""

    def __init__(self, torch, dev, comp, co, cl, want, so, sl):
        self.torch, self.comp, self.co, self.cl, self.want, self.so, self.sl = torch, comp, co, cl, want, so, sl
        self.n = co.numel()
        self.back = torch.full((GUARD + want.numel() + GUARD,), U.FILL, dtype=torch.uint8, device=dev)
        self.out = torch.full((self.n,), U.SENTINEL, dtype=torch.int32, device=dev)

    def launch(self, amd):
        amd.DeviceBatch.decompress_safe(self.comp, self.co, self.cl, self.back[GUARD:], self.so, self.sl, self.out)

    def verdict(self, flags, r):
        """(on the launch's stream) flags[r] = blocks with a wrong out_len, wrong output bytes, written guard bytes; then blank again"""
        torch = self.torch
        m = self.want.numel()
        flags[r, 0] = (self.out != self.sl).sum()
        flags[r, 1] = (self.back[GUARD:GUARD + m] != self.want).sum()
        flags[r, 2] = (self.back[:GUARD] != U.FILL).sum() + (self.back[GUARD + m:] != U.FILL).sum()
        self.back.fill_(U.FILL)
        self.out.fill_(U.SENTINEL)


@pytest.fixture(scope="module")
def victim_and_attacker(amd, dev, ref, corpus):
    """V: 96 blocks per CU (more than the 64 per CU the deep kernel holds at once, fewer than 40960) of 16 KiB App. F data, compressed on
    the device; routes to 0.  K: 40960 blocks, the 32 that decode_route_kernel samples -- blocks ((2 w + k) n) / 32 + n / 64, w = 0 .. 15,
    k = 0, 1: csrc/decode.hip -- the bitmap (near match sources, a stream of 4 KiB and more), every other one the empty block's stream
    `00`; routes to 3, which no candidate kernel of V answers to"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 96 * cus
    assert 64 * cus < n < 40960
    cap = amd.maxCompressedLength(V_BLOCK)
    src = torch.empty(n * V_BLOCK, dtype=torch.uint8, device=dev)
    amd.DeviceBatch.gen_blocks(src, V_BLOCK, V_BLOCK, n, first_idx=7 << 20)
    comp = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
    so = torch.arange(n, dtype=torch.int64, device=dev) * V_BLOCK
    co = torch.arange(n, dtype=torch.int64, device=dev) * cap
    sl = torch.full((n,), V_BLOCK, dtype=torch.int32, device=dev)
    cl = torch.zeros(n, dtype=torch.int32, device=dev)
    amd.DeviceBatch.compress_fast(src, so, sl, comp, co, torch.full((n,), cap, dtype=torch.int32, device=dev), cl)
    torch.cuda.synchronize()
    assert int(cl.min()) >= 4096
    V = Routed(torch, dev, comp, co, cl, src, so, sl)

    pic = corpus["pic[:65536]"]
    s = ref.compress_fast(pic)
    assert len(s) >= 4096 and ref.decompress_safe_raw(s, len(pic))[1][:len(pic)] == pic
    big = set(U.sampled_blocks(K_BLOCKS))
    assert len(big) == 32
    img, k_co, k_cl, k_so, k_sl, p, q = bytearray(), [], [], [], [], 0, 0
    for i in range(K_BLOCKS):
        st, m = (s, len(pic)) if i in big else (b"\x00", 0)
        k_co.append(len(img)); k_cl.append(len(st)); k_so.append(q); k_sl.append(m)
        img += st
        q += m
    i64 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int64)).to(dev)
    i32 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int32)).to(dev)
    K = Routed(torch, dev, torch.frombuffer(bytearray(img + bytes(64)), dtype=torch.uint8).to(dev), i64(k_co), i32(k_cl),
               torch.frombuffer(bytearray(pic * 32), dtype=torch.uint8).to(dev), i64(k_so), i32(k_sl))
    flags = torch.zeros(1, 3, dtype=torch.int64, device=dev)
    for name, L, route in (("V", V, 0), ("K", K, 3)):        # the preconditions, from solo runs
        L.launch(amd)
        L.verdict(flags, 0)
        torch.cuda.synchronize()
        got = amd.last_decode_route()
        assert got[0] == route and got[5] > 0, (name, "routes to", got, "and not to", route)
        assert flags.cpu().tolist() == [[0, 0, 0]], (name, "alone", flags.cpu().tolist())
    yield V, K
    del V, K
    torch.cuda.empty_cache()


@pytest.mark.parametrize("slots", (1, 256))
def test_route_slot_reuse_across_streams(amd, dev, victim_and_attacker, slots):
    """V on S1 and K on S2 back to back, ten times over, then K first: K's route kernel writes 3 while V's later workgroups have yet to
    start and read the word -- with one slot in the ring ("decode_route_slots" 1) on every launch, with the default ring on every
    256th.  A slot's next use is ordered behind its previous user's last candidate kernel: every out_len and every output byte of every
    launch is the source's, the guards are intact"""
    import torch
    V, K = victim_and_attacker
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    fv = torch.full((20, 3), -1, dtype=torch.int64, device=dev)
    fk = torch.full((20, 3), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    amd.set_option("decode_route_slots", slots)
    try:
        for r in range(20):
            order = ((S1, V, fv), (S2, K, fk)) if r < 10 else ((S2, K, fk), (S1, V, fv))
            for S, L, _ in order:
                with torch.cuda.stream(S):
                    L.launch(amd)
            for S, L, f in order:
                with torch.cuda.stream(S):
                    L.verdict(f, r)
        S1.synchronize(); S2.synchronize()
        bad = [(name, r, row) for name, f in (("V", fv), ("K", fk)) for r, row in enumerate(f.cpu().tolist()) if row != [0, 0, 0]]
        assert not bad, ("(launch, round, [blocks with a wrong out_len, wrong bytes, guard bytes written])", len(bad), bad[:6])
    finally:
        torch.cuda.synchronize()
        amd.set_option("decode_route_slots", 256)


# ---- B5 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", sorted(f for f, e in U.TABLE.items() if e.own_scratch))
def test_repeated_calls_in_one_process(amd, dev, case_of, fn):
    """every entry whose scratch the library allocates itself (stream-ordered): 40 identical calls with a device synchronisation
    between them -- where the pool's memory goes back to the system --, then 40 without one; every call's values and bytes against
    the reference"""
    import torch
    run = Run(amd, dev, case_of(fn))
    try:
        run.bring()
        for k in range(40):
            run.blank()
            run.call()
            torch.cuda.synchronize()
            bad = run.problems()
            assert bad == [], (fn, "call", k, "with a synchronisation in front", bad[:4])
        snaps = []
        for k in range(40):
            run.blank()
            run.call()
            snaps.append(run.snapshot())
        torch.cuda.synchronize()
        if run.case.after:          # (the digest is fetched on the host: the last call's)
            snaps = snaps[-1:]
        bad = [(k, p[:3]) for k, s in enumerate(snaps) for p in [run.problems(s)] if p]
        assert not bad, (fn, "calls without a synchronisation between them", len(bad), bad[:4])
    finally:
        torch.cuda.synchronize()
        run.close()
