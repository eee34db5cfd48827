"""The decoders' end-of-block margins on the GPU (-m gpu): the boundary streams of tests/margin_common.py -- a near-maximal simple
sequence at the byte at which an interior loop decides to stay or leave -- through every decoder variant, the batch-size routes, the
partial and dictionary decoders' two kernels, the chain decoder and the decoded-size query.  A wrong margin on the device is a store
past a block's slot into its neighbour's, with no fault: destination slots start at addresses = 0, 1, 127 and 77 (mod 128) with at
least 128 bytes of 0xA5 in front of, between and behind them (a whole staged line, a whole 64-byte step), and every one of those
bytes is checked, with the reference library's return codes and bytes.  tests/test_margin_hostsim.py runs the same cases in the lane
simulator, and shows there that a weakened margin fails them."""
import numpy as np
import pytest

import fast_contract_common as F
import margin_common as M

pytestmark = pytest.mark.gpu

SRC_FRONT, SRC_GAP, SRC_BACK = 4096, 128, 8192   # zeros around the source slots: a wrong read stays inside the allocation
DEVICE = "cuda:0"
PRIMES = (1, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53)


@pytest.fixture(scope="module")
def cs(ref, O):
    return M.CaseSet(ref, O)


def pick(cs, modes):
    idx = [i for i, c in enumerate(cs.cases) if c.mode in modes]
    return [cs.cases[i] for i in idx], [cs.want[i] for i in idx]


class Launch:
    """`replicas` copies of a case list laid out for one device call.  Sources stand once; every replica has destination slots of its
    own (the same layout, a multiple of 128 bytes further on) and its own order of the cases in the launch, so that a case meets other
    neighbours in its wavefront.  rows[k] = (source bytes, slot size, bytes that may be written (<= slot size), return code, expected
    bytes at the slot's start, what the case is)."""

    def __init__(self, rows, replicas=1):
        import torch
        self.torch, self.dev = torch, torch.device(DEVICE)
        n = self.n = len(rows)
        self.rows, self.R = rows, replicas
        src = bytearray(SRC_FRONT)
        so = []
        for r in rows:
            so.append(len(src))
            src += r[0] + bytes(SRC_GAP)
        src += bytes(SRC_BACK)
        self.off, size = M.image([r[1] for r in rows])
        self.rs = size + (-size) % 128
        assert {o % 128 for o in self.off} >= {0, 1, 127} and all(b - a - r[1] >= M.MIN_GUARD for a, b, r in zip(self.off, self.off[1:], rows))
        exp = np.full(self.rs, M.FILL, dtype=np.uint8)
        free = np.zeros(self.rs, dtype=np.bool_)        # bytes a decoder may leave in any state: the rest of a slot behind its result
        for o, (_, slot, room, code, data, _) in zip(self.off, rows):
            assert room <= slot and len(data) <= room
            exp[o:o + len(data)] = np.frombuffer(data, dtype=np.uint8)
            free[o + len(data):o + room] = True
        p = [q for q in PRIMES if q == 1 or n % q][:replicas]
        assert len(p) == replicas or replicas > len(PRIMES)
        order = np.concatenate([(np.arange(n, dtype=np.int64) * p[r % len(p)] + 5 * r) % n for r in range(replicas)])
        self.order = order
        t = lambda a, ty: torch.tensor(np.asarray(a), dtype=ty, device=self.dev)
        self.src = torch.frombuffer(src, dtype=torch.uint8).to(self.dev)
        self.so = t(np.asarray(so, dtype=np.int64)[order], torch.int64)
        self.sl = t(np.asarray([len(r[0]) for r in rows], dtype=np.int32)[order], torch.int32)
        self.do = t(np.asarray(self.off, dtype=np.int64)[order] + np.repeat(np.arange(replicas, dtype=np.int64) * self.rs, n), torch.int64)
        self.slot = t(np.asarray([r[1] for r in rows], dtype=np.int32)[order], torch.int32)
        self.codes = t(np.asarray([r[3] for r in rows], dtype=np.int32)[order], torch.int32)
        self.exp, self.free = torch.from_numpy(exp).to(self.dev), torch.from_numpy(free).to(self.dev)

    def fresh(self):
        torch = self.torch
        dst = torch.full((self.R * self.rs,), M.FILL, dtype=torch.uint8, device=self.dev)
        out = torch.full((self.n * self.R,), -0x5A5A5A, dtype=torch.int32, device=self.dev)
        return dst, out

    def check(self, dst, out, note, codes_only=False):
        torch = self.torch
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        if not torch.equal(out, self.codes):
            bad = torch.nonzero(out != self.codes).flatten()[:6].tolist()
            got = out.cpu().tolist()
            assert False, (note, "return codes", int((out != self.codes).sum()),
                           [(k, int(self.order[k]), self.rows[int(self.order[k])][5], got[k], self.rows[int(self.order[k])][3]) for k in bad])
        if codes_only:
            return
        wrong = (dst.view(self.R, self.rs) != self.exp[None, :]) & ~self.free[None, :]
        if bool(wrong.any()):
            pos = torch.nonzero(wrong)[:4].tolist()
            import bisect
            said = []
            for r, q in pos:
                k = max(bisect.bisect_right(self.off, q) - 1, 0)
                row = self.rows[k]
                said.append(("replica", r, "case", k, row[5], "slot byte", q - self.off[k], "of", row[1], "result", row[3],
                             "accepted output differs" if q - self.off[k] < len(row[4]) else "a byte outside the slot was written"))
            assert False, (note, int(wrong.sum()), said)


def safe_rows(cases, want):
    return [(M.source(c)[0], c.cap, c.cap, w[0], w[1][:max(w[0], 0)], (c.mode, c.tag)) for c, w in zip(cases, want)]


def fast_rows(cases, want):
    return [(M.source(c)[0], c.cap, c.cap, w[0], w[1] if w[0] >= 0 else b"", (c.mode, c.tag)) for c, w in zip(cases, want)]


@pytest.fixture(scope="module")
def safe_all(cs):
    return Launch(safe_rows(*pick(cs, "abch")))


@pytest.fixture(scope="module")
def fast_all(cs):
    return Launch(fast_rows(*pick(cs, "di")))


def run_safe(amd, L, note):
    dst, out = L.fresh()
    amd.DeviceBatch.decompress_safe(L.src, L.so, L.sl, dst, L.do, L.slot, out)
    L.check(dst, out, ("safe",) + tuple(note))


def run_fast(amd, L, note):
    dst, out = L.fresh()
    amd.DeviceBatch.decompress_fast(L.src, L.so, L.sl, dst, L.do, L.slot, out)
    L.check(dst, out, ("fast",) + tuple(note))


@pytest.mark.parametrize("variant", F.DECODE_VARIANTS, ids=lambda v: "lanes%d-pipe%d-stage%d-ring%d" % v)
def test_margins_every_variant(amd, safe_all, fast_all, variant):
    """modes a, b, c and h through the safe decoder and d and i through the fast decoder, one batch of all cases each, one decoder
    variant forced"""
    assert safe_all.n == 3009 + 2209 + 1689 + 350 and fast_all.n == 1689 + 350
    try:
        F.set_knobs(amd, variant)
        run_safe(amd, safe_all, variant)
        run_fast(amd, fast_all, variant)
    finally:
        F.set_knobs(amd, F.DEFAULT_KNOBS)


@pytest.mark.parametrize("per_cu", (5, 16, 33))
def test_margins_batch_size_routes(amd, cs, per_cu):
    """every knob at its default, launches of at most 5 and at most 16 blocks per compute unit (the case list in as many launches as
    that takes) and of more than 32 (the list replicated, every replica in another order): the routes of launch_decompress"""
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    F.set_knobs(amd, F.DEFAULT_KNOBS)
    for rows, run in ((safe_rows(*pick(cs, "abch")), run_safe), (fast_rows(*pick(cs, "di")), run_fast)):
        if per_cu == 33:
            R = -(-(32 * cu + 1) // len(rows))
            L = Launch(rows, replicas=R)
            assert L.n * L.R > 32 * cu
            run(amd, L, ("more than 32 per CU", L.n * L.R, cu))
            continue
        chunk = per_cu * cu
        # (cases of a chunk are taken with a stride, so that every launch has every mode)
        k = -(-len(rows) // chunk)
        for a in range(k):
            part = rows[a::k]
            assert len(part) <= chunk
            run(amd, Launch(part), ("at most %d per CU" % per_cu, len(part), cu, "launch", a))


def test_margins_partial_both_kernels(amd, cs):
    """mode e below 40960 blocks (the deep kernel) and from 40960 on (the staged kernel): the target at the probe's start + d; nothing
    behind min(target, capacity) is written"""
    cases, want = pick(cs, "e")
    rows = [(c.s.data, c.cap, min(c.aux, c.cap), w[0], w[1], (c.mode, c.tag)) for c, w in zip(cases, want)]
    assert len(rows) == 1263
    for R in (1, -(-40960 // len(rows))):
        L = Launch(rows, replicas=R)
        assert (L.n * L.R >= 40960) == (R > 1)
        target = L.torch.tensor(np.asarray([c.aux for c in cases], dtype=np.int32)[L.order % L.n], dtype=L.torch.int32, device=L.dev)
        dst, out = L.fresh()
        amd.DeviceBatch.decompress_safe_partial(L.src, L.so, L.sl, dst, L.do, target, L.slot, out)
        L.check(dst, out, ("partial", L.n * L.R))


def test_margins_dictionary_both_kernels(amd, cs):
    """mode f below 40960 blocks (decode_dict_deep_kernel) and from 40960 on (decode_dict_kernel), dictionaries of 400 and 70000 bytes:
    the probe's match wholly inside the dictionary or straddling the block's start"""
    import torch
    cases, want = pick(cs, "f")
    assert len(cases) == 480
    for dlen in (400, 70000):
        rows = [(c.s.data, c.cap, c.cap, w[0], w[1], (c.mode, c.tag)) for c, w in zip(cases, want) if c.aux == dlen]
        assert len(rows) >= 70
        d = torch.frombuffer(bytearray(cs.dicts[dlen]), dtype=torch.uint8).to(torch.device("cuda", 0))
        for R in (1, -(-40960 // len(rows))):
            L = Launch(rows, replicas=R)
            dst, out = L.fresh()
            amd.DeviceBatch.decompress_safe_dict(L.src, L.so, L.sl, dst, L.do, L.slot, out, d)
            L.check(dst, out, ("dictionary", dlen, L.n * L.R))


def test_margins_chain(amd, cs):
    """mode g: every block as the second of a chain of its own, the probe's match starting in the first block"""
    import torch
    cases, want = pick(cs, "g")
    assert len(cases) == 480
    fb = cs.first_block
    # a chain's region is one slot of the image: 400 bytes of the first block, then the block under test
    rows = [(c.s.data, 400 + c.cap, 400 + c.cap, 0, w[2], (c.mode, c.tag)) for c, w in zip(cases, want)]
    L = Launch(rows)
    n = L.n
    dev = L.dev
    src = torch.cat([L.src, torch.frombuffer(bytearray(fb + bytes(SRC_BACK)), dtype=torch.uint8).to(dev)])
    fb_off = L.src.numel()
    so = torch.stack([torch.full_like(L.so, fb_off), L.so], dim=1).flatten().contiguous()
    sl = torch.stack([torch.full_like(L.sl, len(fb)), L.sl], dim=1).flatten().contiguous()
    cap = torch.stack([torch.full_like(L.slot, 400), L.slot - 400], dim=1).flatten().contiguous()
    first = torch.arange(0, 2 * n + 1, 2, dtype=torch.int32, device=dev)
    dst, _ = L.fresh()
    out = torch.full((2 * n,), -12345, dtype=torch.int32, device=dev)
    cout = torch.full((n,), -1, dtype=torch.int64, device=dev)
    amd.DeviceBatch.decompress_safe_chain(src, so, sl, cap, first, dst, L.do, L.slot.to(torch.int64), out, cout)
    torch.cuda.synchronize()
    got, gc = out.cpu().tolist(), cout.cpu().tolist()
    for k, (c, w) in enumerate(zip(cases, want)):
        assert got[2 * k:2 * k + 2] == w[0] and gc[k] == w[1], (c.tag, got[2 * k:2 * k + 2], w[0], gc[k], w[1])
    L.check(dst, L.codes, ("chain",))


def test_margins_size_query(amd, cs):
    """the decoded-size query on modes a, b, c and h: the reference's return value for every case, in launches of both sizes"""
    rows = safe_rows(*pick(cs, "abch"))
    for R in (1, 3):
        L = Launch(rows, replicas=R)
        _, out = L.fresh()
        amd.DeviceBatch.decoded_size(L.src, L.so, L.sl, L.slot, out)
        L.check(None, out, ("size query", R), codes_only=True)
