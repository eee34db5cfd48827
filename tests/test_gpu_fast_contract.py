"""The fast decoder's bounded-read contract (include/lz4hip.h) in EVERY decode kernel (-m gpu): the SAFE = false halves of the
launchers in csrc/decode_*.hip are device code of their own, and damaged streams reached them only with every knob at its default.
The cases of tests/fast_contract_common.py -- short and long streams, valid, damaged, cut and padded, the committed vectors -- go
through lz4hip_decompress_fast_batch_dev with each forced variant and through each batch-size route, twice: once with 0x00 around
every source slot and 0xA5 around every destination slot, once with 0xFF and 0x5A.  Both runs must give the return code of the
oracle's bounded fast decoder, its bytes where it accepts, and leave every byte outside the destination slots alone; a read behind
src_cap or in front of a destination slot that influences a result shows as a difference between the runs or from the oracle.
(tests/test_fast_contract_hostsim.py runs the same cases in the lane simulator: a case that fails here and passes there is the
device backend's or the instantiation's.)"""
import hashlib

import pytest

import fast_contract_common as F

pytestmark = pytest.mark.gpu

RUNS = ((0x00, 0xA5), (0xFF, 0x5A))   # (fill around the source slots, fill around the destination slots): runs A and B


@pytest.fixture(scope="module")
def cs(ref, O, corpus):
    return F.CaseSet(ref, O, corpus)


class DeviceCases:
    """a case list laid out for the device batch call: the source image of either run, the offset / size tensors, the oracle's codes
    and an image of its accepted output, all on the device and built once"""

    def __init__(self, cases, want):
        import numpy as np
        import torch
        self.torch, self.cases, self.want = torch, cases, want
        dev = torch.device("cuda:0")
        self.src, self.dst = [], []
        for fs, fd in RUNS:
            src, so, sc, dst, do, dl = F.layout(cases, fs, fd)
            self.src.append(torch.frombuffer(bytearray(src), dtype=torch.uint8).to(dev))
            self.dst.append(torch.frombuffer(bytearray(dst), dtype=torch.uint8).to(dev))
        self.total = len(dst)
        self.do_host = do
        i64, i32 = torch.int64, torch.int32
        self.so, self.sc = torch.tensor(so, dtype=i64, device=dev), torch.tensor(sc, dtype=i32, device=dev)
        self.do, self.dl = torch.tensor(do, dtype=i64, device=dev), torch.tensor(dl, dtype=i32, device=dev)
        self.codes = torch.tensor([r for r, _ in want], dtype=i32, device=dev)
        img = np.zeros(self.total, dtype=np.uint8)
        acc = np.zeros(self.total, dtype=np.bool_)
        rej = np.zeros(self.total, dtype=np.bool_)
        for c, (r, d), o in zip(cases, want, do):
            if r >= 0:
                img[o:o + c.dst_len] = np.frombuffer(d, dtype=np.uint8)
                acc[o:o + c.dst_len] = True
            else:
                rej[o:o + c.dst_len] = True      # (a slot's content after a rejection is unspecified)
        self.img, self.acc, self.rej = (torch.from_numpy(a).to(dev) for a in (img, acc, rej))

    def where(self, pos):
        """the case whose destination slot holds or precedes byte `pos` of the destination image"""
        import bisect
        k = max(bisect.bisect_right(self.do_host, pos) - 1, 0)
        c = self.cases[k]
        return "byte %d = slot %d %+d (%s, src_cap %d, stream bytes %d, dst_len %d, expected %d)" % (
            pos, k, pos - self.do_host[k], c.kind, len(c.slot), c.body, c.dst_len, self.want[k][0])

    def run(self, amd, which, note):
        """one launch on the images of run `which`; asserts codes, accepted bytes, everything outside the slots, the source image"""
        torch = self.torch
        fs, fd = RUNS[which]
        src = self.src[which]
        keep = src.clone()
        dst = self.dst[which].clone()
        out = torch.full((len(self.cases),), -0x5A5A5A, dtype=torch.int32, device=src.device)
        amd.DeviceBatch.decompress_fast(src, self.so, self.sc, dst, self.do, self.dl, out)
        torch.cuda.synchronize()
        note = (note() if callable(note) else note, "run " + "AB"[which])
        if not torch.equal(out, self.codes):
            bad = torch.nonzero(out != self.codes).flatten()[:6].tolist()
            got = out.cpu().tolist()
            assert False, (note, "return codes", [(k, self.cases[k].kind, len(self.cases[k].slot), self.cases[k].body, self.cases[k].dst_len,
                                                   got[k], self.want[k][0]) for k in bad])
        exp = torch.where(self.acc, self.img, torch.full_like(self.img, fd))
        wrong = (dst != exp) & ~self.rej
        if bool(wrong.any()):
            pos = torch.nonzero(wrong).flatten()[:4].tolist()
            assert False, (note, "accepted output differs from the oracle's" if bool(self.acc[pos[0]]) else "a byte outside every slot does not hold its fill",
                           int(wrong.sum()), [self.where(p) for p in pos])
        assert torch.equal(src, keep), (note, "the source image was written")
        return out, dst

    def run_both(self, amd, note):
        (oa, da), (ob, db) = self.run(amd, 0, note), self.run(amd, 1, note)
        assert self.torch.equal(oa, ob), (note, "the runs' return codes differ")
        differ = (da != db) & self.acc
        assert not bool(differ.any()), (note, "the runs' accepted output differs", [self.where(p) for p in self.torch.nonzero(differ).flatten()[:4].tolist()])


@pytest.fixture(scope="module")
def all_cases(cs):
    return DeviceCases(cs.cases, cs.want)


@pytest.mark.parametrize("variant", F.DECODE_VARIANTS, ids=lambda v: "lanes%d-pipe%d-stage%d-ring%d" % v)
def test_every_loop(amd, all_cases, variant):
    """every case in one batch through the SAFE = false instantiation of one decoder variant, runs A and B"""
    try:
        F.set_knobs(amd, variant)
        all_cases.run_both(amd, variant)
    finally:
        F.set_knobs(amd, F.DEFAULT_KNOBS)


def routed_order(pool, n, sampled):
    """n indices into `pool` (repeating it as often as that takes) with the `sampled` ones -- cases long enough for the route sampler
    of csrc/decode.hip to read: it looks into blocks j n / 32 + n / 64, j = 0 .. 31 -- moved to where it looks"""
    order = [i % pool for i in range(n)]
    for j in range(32):
        pos, s = j * n // 32 + n // 64, sampled[j % len(sampled)]
        at = order.index(s)
        order[pos], order[at] = order[at], order[pos]
    return order


def test_batch_size_routes(amd, cs):
    """every knob at its default: the batch sizes at which launch_decompress takes another way -- up to 5 blocks per compute unit the
    trio loop, up to 16 the parallel wave loop, beyond that the decoder is chosen on the device (decode_route_kernel), with a rule of
    its own for batches of up to 32 blocks per CU; the routed batches with decode_route_short at its default, 255 (the wave kernel for
    whatever is near) and 0 (never).  The sampler's fast-decoder rule looks a fifth of dst_len into a slot whose length it does not
    know: long cases, damaged ones among them, stand where it samples."""
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    # launch order of this test: the long cases first, so that every batch has all of them
    idx = list(range(len(cs.short), len(cs.short) + len(cs.long))) + list(range(len(cs.short))) + list(range(len(cs.short) + len(cs.long), len(cs.cases)))
    pool = [cs.cases[i] for i in idx]
    want = [cs.want[i] for i in idx]
    N = len(pool)
    sampled = [k for k in range(len(cs.long)) if len(pool[k].slot) >= 8192 and pool[k].dst_len >= 5 * 4096]
    assert len(sampled) >= 32
    sampled = sampled[::len(sampled) // 32][:32]

    def batch(order):
        return DeviceCases([pool[i] for i in order], [want[i] for i in order])
    sizes = {"trio": 5 * cu, "parallel wave": min(max(N, 5 * cu + 1), 16 * cu),
             "routed, small": min(max(N, 16 * cu + 1), 32 * cu), "routed": max(2 * N, 32 * cu + 1)}
    assert 5 * cu < sizes["parallel wave"] and 16 * cu < sizes["routed, small"] <= 32 * cu < sizes["routed"]
    F.set_knobs(amd, F.DEFAULT_KNOBS)
    for name in ("trio", "parallel wave"):
        batch([i % N for i in range(sizes[name])]).run_both(amd, (name, sizes[name], cu))
    try:
        for name in ("routed, small", "routed"):
            b = batch(routed_order(N, sizes[name], sampled))
            for short in (-1, 255, 0):
                if short >= 0:
                    amd.set_option("decode_route_short", short)
                b.run_both(amd, lambda: (name, sizes[name], cu, "decode_route_short", short, "last_decode_route", amd.last_decode_route()))
            amd.set_option("decode_route_short", 8)
            del b
    finally:
        amd.set_option("decode_route_short", 8)


@pytest.mark.parametrize("variant", F.DECODE_VARIANTS, ids=lambda v: "lanes%d-pipe%d-stage%d-ring%d" % v)
def test_committed_vectors_every_loop(amd, cs, variant):
    """tests/test_gpu_scale.py::test_fast_decoder_contract_pinned's check -- the committed return codes, the sha256 of every accepted
    output, the byte behind every slot -- through every decoder variant instead of the default alone"""
    import torch
    dev = torch.device("cuda:0")
    src, so, sc, dst, do, dl = F.layout(cs.vectors, 0x77, 0xA5)
    t = lambda v, ty: torch.tensor(v, dtype=ty, device=dev)
    d = torch.frombuffer(bytearray(dst), dtype=torch.uint8).to(dev)
    out = torch.full((len(so),), -0x5A5A5A, dtype=torch.int32, device=dev)
    try:
        F.set_knobs(amd, variant)
        amd.DeviceBatch.decompress_fast(torch.frombuffer(bytearray(src), dtype=torch.uint8).to(dev), t(so, torch.int64), t(sc, torch.int32),
                                        d, t(do, torch.int64), t(dl, torch.int32), out)
        torch.cuda.synchronize()
    finally:
        F.set_knobs(amd, F.DEFAULT_KNOBS)
    got, host = out.cpu().tolist(), d.cpu().numpy().tobytes()
    for k, (c, (ret, _), sha, r, o) in enumerate(zip(cs.vectors, cs.vector_want, cs.vector_sha, got, do)):
        assert r == ret, (variant, k, c.slot[:20].hex(), len(c.slot), c.dst_len, r, ret)
        if ret >= 0:
            assert hashlib.sha256(host[o:o + c.dst_len]).hexdigest() == sha, (variant, k)
        assert host[o + c.dst_len:o + c.dst_len + F.DST_GUARD] == b"\xA5" * F.DST_GUARD, (variant, k, "bytes behind the slot were written")
    assert host[:F.DST_FRONT] == b"\xA5" * F.DST_FRONT
