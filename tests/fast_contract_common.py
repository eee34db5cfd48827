"""Shared pieces of the fast decoder's bounded-read contract tests (test_fast_contract_hostsim.py, test_gpu_fast_contract.py): the
decoder variant list, the cases -- a source SLOT of exactly src_cap bytes and a decoded size --, what the oracle's bounded fast
decoder makes of them, and the two host images a device batch is launched on.

include/lz4hip.h: lz4hip_decompress_fast* reads nothing beyond src_cap[i] bytes of a block's source slot, nothing in front of its
destination slot, writes nothing outside it, and rejects a stream that would need such an access with -(input position) - 1.  A
read that breaks this cannot be seen; one that changes a result can -- so every case decodes twice, with different bytes around
its slots, and both runs must give what O.decompress_fast_bounded gives of the slot alone."""
import hashlib
import json
import os
import random
from typing import NamedTuple

from conftest import GOLD, deep_decoder_cases, lz4_seq, ring_edge_stream, rnd_inputs, wild_piece_stream

# (decode_lanes, decode_pipe, decode_stage, decode_ring): every decoder kernel the launchers instantiate.  pipe 1: the pipelined
# interior loop; stage: output staging in LDS (plain loop only); pipe 2: the deep loop (lz4_decode_deep.h); pipe 3: the ring loop
# (lz4_decode_ring.h; (4, 3, 2048) is the routed default of 16384 .. 40959 big blocks); pipe 4: the wave loop (lz4_decode_wave.h), a
# wavefront per block; pipe 5: its parallel form; pipe 7: the pair loop (lz4_decode_pair.h); pipe 8: the trio loop (lz4_decode_trio.h)
DECODE_VARIANTS = ((0, -1, -1, 0), (4, 0, 0, 0), (4, 1, 0, 0), (8, 1, 0, 0), (16, 0, 0, 0), (64, 0, 0, 0), (64, 1, 0, 0), (4, 0, 1, 0), (8, 0, 1, 0),
                   (32, 0, 1, 0), (64, 0, 1, 0),
                   (4, 2, 0, 0), (8, 2, 0, 0), (16, 2, 0, 0),
                   (1, 3, 0, 256), (1, 3, 0, 512), (4, 3, 0, 512), (4, 3, 0, 1024), (4, 3, 0, 2048), (8, 3, 0, 512), (8, 3, 0, 4096), (16, 3, 0, 4096),
                   (64, 4, 0, 0), (64, 4, 0, 8192), (64, 4, 0, 16384), (64, 4, 0, 32768), (64, 4, 0, 65536),
                   (64, 5, 0, 0), (64, 5, 0, 8192), (64, 5, 0, 16384), (64, 5, 0, 32768), (64, 5, 0, 65536),
                   (64, 7, 0, 0), (64, 7, 0, 16384), (64, 7, 0, 32768), (64, 7, 0, 65536),
                   (64, 8, 0, 0), (64, 8, 0, 8192), (64, 8, 0, 16384), (64, 8, 0, 32768), (64, 8, 0, 65536))
DEFAULT_KNOBS = (0, -1, -1, 0)

SHORT_INPUT_SEED, SHORT_DAMAGE_SEED, LONG_SEED = 2026, 2027, 31
SRC_FRONT, SRC_BACK, SRC_GAPS = 4096, 8192, (1, 3, 17, 64)   # source image: fill in front, behind, and between the slots (rotating)
DST_FRONT, DST_GUARD = 256, 41                               # destination image: fill in front of the first slot, between and behind


class Case(NamedTuple):
    slot: bytes      # exactly src_cap bytes: the stream, cut or padded
    dst_len: int
    body: int        # how many bytes of the slot are the stream's; slot[body:] is padding
    kind: str
    whole: bool      # the slot holds the whole stream (src_cap >= its length)


def set_knobs(amd, knobs):
    for name, v in zip(("decode_lanes", "decode_pipe", "decode_stage", "decode_ring"), knobs):
        amd.set_option(name, v)


def _slot(stream, src_cap, rng, pad=None):
    """the stream cut or padded to src_cap bytes; the padding is 0x00, 0xFF or random bytes (`pad`: 0 / 1 / 2, else drawn)"""
    pad = rng.randrange(3) if pad is None else pad
    extra = src_cap - len(stream)
    if extra <= 0:
        return bytes(stream[:src_cap]), src_cap, extra == 0
    fill = bytes(extra) if pad == 0 else b"\xFF" * extra if pad == 1 else rng.randbytes(extra)
    return bytes(stream) + fill, len(stream), True


def repadded(case, byte):
    """the case with its in-slot padding replaced by `byte`"""
    return case._replace(slot=case.slot[:case.body] + bytes([byte]) * (len(case.slot) - case.body))


def short_cases(ref, O, corpus, count=4000):
    """`count` inputs of at most 30000 bytes compressed by the reference library, in the six forms of
    test_gpu_parity.py::test_decode_fuzz_bit_exact: as is, wrong dst_len, flipped bytes, truncated, extended, random bytes"""
    rng = random.Random(SHORT_DAMAGE_SEED)
    out = []
    for v in rnd_inputs(O, corpus, SHORT_INPUT_SEED, count, max_n=30000):
        c = bytearray(ref.compress_fast(v))
        mode, n = rng.randrange(6), len(v)
        if mode == 1:
            n = max(0, len(v) + rng.choice([-1, 1, -5, 5, -12, 12, -33, 33, 64, 100]))
        elif mode == 2 and c:
            for _ in range(rng.randrange(1, 4)):
                c[rng.randrange(len(c))] = rng.randrange(256)
        elif mode == 3 and len(c) > 1:
            c = c[:rng.randrange(1, len(c))]
        elif mode == 4:
            c = c + rng.randbytes(rng.randrange(1, 20))
        elif mode == 5:
            c, n = bytearray(rng.randbytes(rng.randrange(1, 40))), rng.randrange(0, 200)
        src_cap = max(0, len(c) + rng.choice([0, 0, 0, 3, 16, 64, -1, -2, -7]))
        slot, body, whole = _slot(c, src_cap, rng)
        out.append(Case(slot, n, body, ("valid", "dst_len", "flipped", "truncated", "extended", "random")[mode], whole))
    return out


def _long_damage(valid, rng):
    """conftest.deep_decoder_cases' damage: every valid stream, then each with flipped bytes (three times), truncated, with too small
    and too big a decoded size"""
    cases = [(c, n, "valid") for c, n in valid]
    for c, n in valid:
        for _ in range(3):
            b = bytearray(c)
            for _ in range(rng.randrange(1, 4)):
                b[rng.randrange(len(b))] = rng.randrange(256)
            cases.append((bytes(b), n, "flipped"))
        cases.append((c[:rng.randrange(len(c) // 2, len(c))], n, "truncated"))
        cases.append((c, n - rng.randrange(1, 700), "dst_len"))
        cases.append((c, n + rng.randrange(1, 100), "dst_len"))
    return cases


def long_cases(ref, O, corpus):
    """streams long enough for every interior loop to run: conftest.deep_decoder_cases (valid and damaged), then eight streams each
    of conftest.wild_piece_stream and conftest.ring_edge_stream with the same damage.  -> (cases, how many come from
    deep_decoder_cases: those lead the list)"""
    rng = random.Random(LONG_SEED)
    valid, deep = deep_decoder_cases(ref, O, corpus, rng, lz4_seq)
    out = []

    def add(raw):
        for c, n, kind in raw:
            src_cap = max(0, len(c) + rng.choice([0, 0, 5, 64, -1, -3, -40, -700]))
            slot, body, whole = _slot(c, src_cap, rng)
            out.append(Case(slot, n, body, "long " + kind, whole))
    add([(c, n, "valid" if k < len(valid) else "damaged") for k, (c, n) in enumerate(deep)])
    hand = [wild_piece_stream(1 << (13 + k % 4), rng) for k in range(8)] + [ring_edge_stream(rng, rng.choice([20000, 90000, 150000])) for _ in range(8)]
    add(_long_damage(hand, rng))
    return out, len(deep)


def contract_vectors():
    """the 600 committed vectors of tests/golden/fast_decode_contract.json -> (cases, their committed return codes, sha256 of the
    accepted ones' output (None for a rejected one))"""
    vecs = json.load(open(os.path.join(GOLD, "fast_decode_contract.json")))["cases"]
    cases, rets, shas = [], [], []
    for e in vecs:
        c = bytes.fromhex(e["hex"])
        body = min(len(c), e["src_cap"])
        cases.append(Case(c[:e["src_cap"]] + bytes(max(0, e["src_cap"] - len(c))), e["dst_len"], body, "vector", len(c) <= e["src_cap"]))
        rets.append(e["ret"]); shas.append(e["sha256"] if e["ret"] >= 0 else None)
    return cases, rets, shas


def expected(O, cases):
    """[(return code, dst_len bytes)] of the oracle's bounded fast decoder, given the slot alone"""
    return [O.decompress_fast_bounded(c.slot, len(c.slot), c.dst_len) for c in cases]


def near_cap(case, ret, within=16):
    """a rejection at an input position within `within` bytes of src_cap"""
    return ret < 0 and len(case.slot) - (-ret - 1) <= within


# Cases that once made a device kernel differ from the oracle while the lane simulator agreed (none so far).  A fixed case is kept
# here by name and joins every test of both files: name -> Case.
NAMED_CASES = {}


class CaseSet:
    """the whole case list in launch order -- short, long, committed vectors, named -- with the expected results, computed once"""

    def __init__(self, ref, O, corpus):
        self.short = short_cases(ref, O, corpus)
        self.long, self.n_deep = long_cases(ref, O, corpus)
        self.vectors, vec_ret, self.vector_sha = contract_vectors()
        self.named = list(NAMED_CASES.values())
        self.short_want = expected(O, self.short)
        self.long_want = expected(O, self.long)
        vec_want = expected(O, self.vectors)
        # the vectors' expected results come from the FILE: the return code as committed, the bytes checked against its sha256
        for k, ((r, d), fr, sh) in enumerate(zip(vec_want, vec_ret, self.vector_sha)):
            assert r == fr and (sh is None or hashlib.sha256(d).hexdigest() == sh), ("the oracle left the committed vector", k, r, fr)
        self.vector_want = [(fr, d) for (r, d), fr in zip(vec_want, vec_ret)]
        self.cases = self.short + self.long + self.vectors + self.named
        self.want = self.short_want + self.long_want + self.vector_want + expected(O, self.named)


def layout(cases, fill_src, fill_dst):
    """The two host images of a device batch and its offset / size lists: (src image, src_off, src_cap, dst image, dst_off, dst_len).
    Source: SRC_FRONT bytes of fill_src, each slot followed by a gap of fill_src of rotating length, SRC_BACK bytes behind -- so much
    that even a wrong read of a whole stream-ring step stays inside the allocation (these tests look for wrong bytes; they must not
    fault the device).  Destination: all fill_dst, DST_FRONT bytes in front, DST_GUARD bytes between and behind the slots."""
    src = bytearray(bytes([fill_src]) * SRC_FRONT)
    so, sc, do, dl, q = [], [], [], [], DST_FRONT
    for k, c in enumerate(cases):
        so.append(len(src)); sc.append(len(c.slot))
        src += c.slot
        src += bytes([fill_src]) * SRC_GAPS[k % len(SRC_GAPS)]
        do.append(q); dl.append(c.dst_len)
        q += c.dst_len + DST_GUARD
    src += bytes([fill_src]) * SRC_BACK
    return bytes(src), so, sc, bytes([fill_dst]) * q, do, dl
