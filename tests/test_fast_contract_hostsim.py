"""The fast decoder's bounded-read contract without a GPU: that the case set of tests/fast_contract_common.py is what it claims to be
(the GPU test, test_gpu_fast_contract.py, must not pass on cases that say nothing), that the oracle's bounded fast decoder keeps the
contract itself, that it is liblz4's LZ4_decompress_fast on undamaged streams, and that one loop of every decoder family agrees with
it in the lane simulator in fast mode -- which is what tells a mismatch on the device apart as the device backend's."""
import pytest

import fast_contract_common as F
from test_hostsim import load_sim, sim_decode, wave_flag


@pytest.fixture(scope="module")
def cs(ref, O, corpus):
    return F.CaseSet(ref, O, corpus)


@pytest.fixture(scope="module")
def sim():
    return load_sim()


def test_case_set_is_what_it_claims(cs, O):
    """enough accepted and rejected cases, enough rejections right at src_cap (where a bound off by a few bytes shows), and enough
    cases whose result depends on the bytes of the slot behind the stream: those are the ones in which a decoder that reads the bytes
    BEHIND the slot instead gives itself away between the two runs of the GPU test.  (Counts for the committed seeds: short 4000
    cases, 1408 accepted, 2592 rejected, 1518 of them within 16 bytes of src_cap; the deep_decoder_cases part of the long ones 147,
    39, 108, 49 -- all 259 long ones: 102 --; 218 short and 13 long results depend on the in-slot padding.)"""
    short_ret = [r for r, _ in cs.short_want]
    deep_ret = [r for r, _ in cs.long_want[:cs.n_deep]]
    assert len(cs.short) == 4000 and cs.n_deep == 147 and len(cs.long) == 147 + 16 * 7 and len(cs.vectors) == 600
    for name, rets in (("short", short_ret), ("long (deep_decoder_cases)", deep_ret), ("long", [r for r, _ in cs.long_want]), ("all", [r for r, _ in cs.want])):
        acc = sum(r >= 0 for r in rets)
        print(name, "total", len(rets), "accepted", acc, "rejected", len(rets) - acc)
        if name != "long":   # (printed only: the hand-assembled streams' damaged forms outnumber their valid ones six to one)
            assert 4 * acc >= len(rets) and 4 * (len(rets) - acc) >= len(rets), (name, acc, len(rets))
    near_short = sum(F.near_cap(c, r) for c, r in zip(cs.short, short_ret))
    near_long = sum(F.near_cap(c, r) for c, (r, _) in zip(cs.long, cs.long_want))
    near_deep = sum(F.near_cap(c, r) for c, r in zip(cs.long[:cs.n_deep], deep_ret))
    print("rejected within 16 bytes of src_cap: short", near_short, "long", near_long, "(deep_decoder_cases part", near_deep, ")")
    assert near_short >= 1000 and near_long >= 30 and near_deep >= 30
    dep = {}
    for name, cases in (("short", cs.short), ("long", cs.long)):
        padded = [c for c in cases if len(c.slot) > c.body]
        a = F.expected(O, [F.repadded(c, 0x00) for c in padded])
        b = F.expected(O, [F.repadded(c, 0xFF) for c in padded])
        dep[name] = sum(x[0] != y[0] or (x[0] >= 0 and x[1] != y[1]) for x, y in zip(a, b))
    print("results that depend on the in-slot padding:", dep)
    assert dep["short"] + dep["long"] >= 100 and dep["short"] >= 100


def test_oracle_keeps_its_own_contract(cs, O):
    """the oracle's result is a function of the slot alone: 64 bytes of 0x00 or of 0xFF behind src_cap change nothing"""
    differ = 0
    for c, (r, d) in zip(cs.cases, cs.want):
        a = O.decompress_fast_bounded(c.slot + bytes(64), len(c.slot), c.dst_len)
        b = O.decompress_fast_bounded(c.slot + b"\xFF" * 64, len(c.slot), c.dst_len)
        differ += not (a[0] == b[0] == r and (r < 0 or a[1] == b[1] == d))
    assert differ == 0, differ


def test_undamaged_streams_agree_with_liblz4(cs, ref):
    """an undamaged stream with its exact decoded size in a slot that holds all of it: LZ4_decompress_fast's return value and bytes"""
    seen = 0
    for c, (r, d) in zip(cs.short + cs.long, cs.short_want + cs.long_want):
        if c.kind.endswith("valid") and c.whole:
            rr, rd = ref.decompress_fast_raw(c.slot[:c.body], c.dst_len)
            assert (r, d) == (rr, rd) and r == c.body, (c.kind, len(c.slot), c.body, c.dst_len, r, rr)
            seen += 1
    assert seen >= 400, seen


SIM_LOOPS = {
    "plain 4": 4, "pipelined 8": 8 | 0x100, "staged 8": 8 | 0x200, "plain 64": 64, "deep 8": 8 | 0x400,
    "ring (4, 2 KiB)": 4 | 0x800 | (11 << 12), "ring (1, 256)": 1 | 0x800 | (8 << 12),
    "wave 8 KiB": wave_flag(13), "parallel wave 8 KiB": wave_flag(13, par=True), "parallel wave 64 KiB": wave_flag(16, par=True),
    "pair 16 KiB": wave_flag(14, par="pair"), "trio 8 KiB": wave_flag(13, par="trio"), "trio 64 KiB": wave_flag(16, par="trio"),
}


@pytest.mark.parametrize("loop", list(SIM_LOOPS))
def test_lane_simulator_agrees_in_fast_mode(cs, sim, loop):
    """every long case, 1200 short ones and the named ones through one loop of each decoder family in the lock-step simulator,
    SAFE = false, the destination slot 0 / 3 / 64 bytes into its buffer: the oracle's return code, and its bytes where it accepts.
    (The simulator fails a decode on any access outside the block's slots.)"""
    flag = SIM_LOOPS[loop]
    step = len(cs.short) // 1200
    todo = list(zip(cs.long, cs.long_want)) + list(zip(cs.short[::step][:1200], cs.short_want[::step][:1200])) + \
        list(zip(cs.named, cs.want[len(cs.want) - len(cs.named):]))
    bad = []
    for k, (c, (r, d)) in enumerate(todo):
        shift = (0, 3, 64)[(k + len(loop)) % 3]
        r4, d4 = sim_decode(sim, c.slot, c.dst_len, 0, flag, src_size=len(c.slot), shift=shift)
        if r4 != r or (r >= 0 and d4[:c.dst_len] != d):
            bad.append((k, c.kind, len(c.slot), c.body, c.dst_len, shift, r4, r))
    assert not bad, (loop, len(bad), bad[:5])
