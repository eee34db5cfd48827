"""Shared pieces of the stream-contract tests (test_userstream_table.py on the CPU, test_gpu_user_streams.py on the GPU): every device
entry point of include/lz4hip.h takes a `void* stream`, and the header promises that the work is enqueued on it and that the call
returns without waiting for it -- apart from the entries it names.  TABLE has one entry per lz4hip_*_dev* function with the call that
reaches it, a small case builder, the source of the expected values and what the header says about synchronisation;
test_userstream_table.py fails when the header declares a function that is in neither TABLE nor EXEMPT, or says something else about it.

A CASE is one call, small: about 40 blocks of 0 .. 70000 bytes (text, App. F, random) at odd offsets, every destination slot with
GUARD bytes of 0xA5 on either side.  It comes with a DECOY: an input X of the same offsets, lengths and capacities as the real input Y
and other bytes, so that work which runs before the stream has brought Y in, or after the snapshot was taken, shows as X's result or
as nothing at all.  The device arrays of offsets, lengths and capacities have decoys too (zeros: whatever reads them too early reads
nothing and writes nothing).

Expected values come from the reference library (`ref`, RefMore and the helpers of the other *_common modules) and, for the fast
decoder and the block generator, from the oracle port -- never from this project's output."""
import random
import re
from typing import Callable, NamedTuple, Optional

import far_common as F

SIZES = (0, 1, 12, 13, 64, 1000, 4096, 65536, 65546, 65547, 70000)
GUARD = 41
FILL = 0xA5
SENTINEL = -12345              # what every result array holds before a call
DICT_LEN = 4096
HC_LEVEL = 4               # (the hash-chain strategy with lazy evaluation, at a depth that keeps 80 calls of B5 within seconds)
ACCEL = 4
CONTAINER_BLOCK = 4096
GEN_LEN, GEN_BLOCKS, GEN_FIRST = 1000, 40, 5


class Slot(NamedTuple):
    """dst[at, at + own) belongs to one block: `out` = the reference's bytes at its start (None: open, e.g. a failed block), x_out = what
    the decoy would give there"""
    name: str
    at: int
    own: int
    out: Optional[bytes]
    x_out: Optional[bytes]
    src_n: int = 1           # the block's input bytes (0: the decoy has nothing to differ in)


class Case(NamedTuple):
    src_y: bytes
    src_x: bytes
    ins: dict                    # name -> (numpy dtype name, the real values, the decoy values): the device arrays the entry reads
    dst_len: int
    slots: list                  # [Slot]
    outs: dict                   # name -> (numpy dtype name, the reference's values, the decoy's values): the arrays the entry writes
    call: Callable               # call(amd, t): the entry point on the tensors t[name] (src, dst, the arrays) and on what setup made
    setup: Optional[Callable] = None      # setup(amd, torch, dev) -> {name: object} added to t (a dictionary handle, a workspace)
    teardown: Optional[Callable] = None   # teardown(t)
    after: Optional[Callable] = None      # after(amd, t) -> {name: values}: results fetched on the host once the stream is done (a digest)
    check: Optional[Callable] = None      # check(dst bytes, {name: values}) -> [problems] in place of the slot-by-slot comparison


def blocks(O, corpus):
    """[(name, y, x)]: text, App. F and random bytes of every size of SIZES, and for each the decoy of the same length"""
    b = corpus["book1[:200000]"]
    out = []
    for k, n in enumerate(SIZES):
        for kind, y, x in (("text", b[:n], b[100001:100001 + n]), ("App. F", O.gen_block(n, 1 + k), O.gen_block(n, 101 + k)),
                           ("random", random.Random(50 + k).randbytes(n), random.Random(150 + k).randbytes(n))):
            if n and x[0] == y[0]:          # (a block of one byte has nothing else to differ in)
                x = bytes([x[0] ^ 0xFF]) + x[1:]
            out.append(("%s %d" % (kind, n), y, x))
    return out


def flipped(s):
    """the decoy of a compressed stream: the same length, no byte the same"""
    return bytes(v ^ 0x5A for v in s)


class Layout:
    """sources at odd offsets with a few bytes between them, slots at odd offsets with GUARD bytes around each"""

    def __init__(self):
        self.src_y, self.src_x, self.dst_len = bytearray(b"\x33"), bytearray(b"\xCC"), GUARD | 1

    def source(self, y, x):
        assert len(y) == len(x)
        if not len(self.src_y) & 1:
            self.src_y += b"\x33"; self.src_x += b"\xCC"
        at = len(self.src_y)
        self.src_y += y + b"\x33\x33\x33"; self.src_x += x + b"\xCC\xCC\xCC"
        return at

    def slot(self, own):
        at = self.dst_len | 1
        self.dst_len = at + own + GUARD
        return at

    def tail(self):
        """room behind the last source: a decoy offset of 0 with a real length stays inside the buffer, and decoders read ahead"""
        self.src_y += b"\x33" * 128; self.src_x += b"\xCC" * 128
        return bytes(self.src_y), bytes(self.src_x)


def _block_case(items, xs, x_result, call, second=None, setup=None, teardown=None, has_dst=True, p2_in=None):
    """the common shape: items = [(name, data, own, p1, ret, out, p2)] as far_common's item builders make them, xs = the decoy of each
    item's data, x_result(x, item) -> (ret, bytes or None, ret2) = the reference on the decoy (None: a case without a stated decoy).  `second` names the second result array
    (destSize: the input consumed), p2_in a second input array (the partial decoder: the capacity)"""
    lay = Layout()
    src_off, slots, ret_x, ret2_x = [], [], [], []
    for it, x in zip(items, xs):
        name, data, own, p1, ret, out, p2 = it
        src_off.append(lay.source(data, x))
        rx, bx, r2x = x_result(x, it) if x_result else (None, None, None)
        ret_x.append(rx); ret2_x.append(r2x)
        if has_dst:
            slots.append(Slot(name, lay.slot(own), own, out, bx, len(data)))
    n = len(items)
    src_y, src_x = lay.tail()
    assert len(src_y) > max(len(it[1]) for it in items)
    ins = {"src_off": ("int64", src_off, [0] * n), "src_len": ("int32", [len(it[1]) for it in items], [0] * n),
           "p1": ("int32", [it[3] for it in items], [0] * n)}
    if has_dst:
        ins["dst_off"] = ("int64", [s.at for s in slots], [s.at for s in slots])
    if p2_in:
        ins[p2_in] = ("int32", [it[6] for it in items], [0] * n)
    outs = {"out": ("int32", [it[4] for it in items], ret_x if x_result else None)}
    if second:
        outs[second] = ("int32", [it[6] for it in items], ret2_x if x_result else None)
    return Case(src_y, src_x, ins, lay.dst_len if has_dst else 0, slots, outs, call, setup, teardown)


def _common(method, **kw):
    """DeviceBatch.<method>(src, src_off, src_len, dst, dst_off, p1, out, **kw)"""
    def call(amd, t):
        extra = {k: (t[v[1:]] if isinstance(v, str) and v.startswith("@") else v) for k, v in kw.items()}
        getattr(amd.DeviceBatch, method)(t["src"], t["src_off"], t["src_len"], t["dst"], t["dst_off"], t["p1"], t["out"], **extra)
    return call


def _dest(method, **kw):
    def call(amd, t):
        getattr(amd.DeviceBatch, method)(t["src"], t["src_off"], t["src_len"], t["dst"], t["dst_off"], t["p1"], t["out"], t["consumed"], **kw)
    return call


def _one_cap_each(blks, fn):
    """far_common.compress_items gives every block at the bound, at the reference's size and one byte below it: here block k takes the
    k-th of the three in turn"""
    return [F.compress_items([(name, y)], fn)[k % 3] for k, (name, y, _) in enumerate(blks)]


def _compress(ref, O, corpus, fn, call, most=None, **kw):
    blks = [b for b in blocks(O, corpus) if most is None or len(b[1]) <= most]

    def x_result(x, it):
        r, by = fn(x, it[3])
        return r, by if r > 0 else None, 0
    return _block_case(_one_cap_each(blks, fn), [x for _, _, x in blks], x_result, call, **kw)


def compress_fast_case(ref, O, corpus):
    return _compress(ref, O, corpus, ref.compress_fast_raw, _common("compress_fast"))


def compress_accel_case(ref, O, corpus):
    rm = F.RefMore(ref)
    return _compress(ref, O, corpus, lambda v, cap: rm.accel(v, cap, ACCEL), _common("compress_fast", acceleration=ACCEL))


def compress_hc_case(ref, O, corpus, method="compress_hc"):
    return _compress(ref, O, corpus, lambda v, cap: ref.compress_hc_raw(v, HC_LEVEL, cap), _common(method, level=HC_LEVEL))


def compress_hc_sync_case(ref, O, corpus):
    return compress_hc_case(ref, O, corpus, "compress_hc_sync")


def compress_hc_sync_small_case(ref, O, corpus):
    """the blocks of up to 4 KiB only: a call whose kernels take a few milliseconds"""
    return _compress(ref, O, corpus, lambda v, cap: ref.compress_hc_raw(v, HC_LEVEL, cap), _common("compress_hc_sync", level=HC_LEVEL), most=4096)


def _dest_case(ref, O, corpus, full, fn, call):
    """far_common.dest_items gives every block at targets below, at and above its full size: block k takes the k-th in turn"""
    blks = blocks(O, corpus)
    items = []
    for k, (name, y, _) in enumerate(blks):
        its = F.dest_items([(name, y)], full, fn)
        items.append(its[k % len(its)])

    def x_result(x, it):
        r, cons, by = fn(x, it[3])
        return r, by, cons
    return _block_case(items, [x for _, _, x in blks], x_result, call, second="consumed")


def dest_size_case(ref, O, corpus):
    rm = F.RefMore(ref)
    return _dest_case(ref, O, corpus, lambda v: len(ref.compress_fast(v)), rm.dest_size, _dest("compress_dest_size"))


def hc_dest_size_case(ref, O, corpus, method="compress_hc_dest_size"):
    rm = F.RefMore(ref)
    return _dest_case(ref, O, corpus, lambda v: ref.compress_hc_raw(v, HC_LEVEL, F.bound(len(v)))[0], lambda v, t: rm.hc_dest_size(v, t, HC_LEVEL),
                      _dest(method, level=HC_LEVEL))


def hc_dest_size_sync_case(ref, O, corpus):
    return hc_dest_size_case(ref, O, corpus, "compress_hc_dest_size_sync")


def _with_dictionary(amd, torch, dev):
    return {"dic": amd.LZ4Dictionary(F.dict_of(DICT_LEN))}


def _close_dictionary(t):
    t["dic"].close()


def compress_dict_case(ref, O, corpus):
    from dict_common import RefDict
    from dictc_common import ref_compress
    rd, d = RefDict(ref), F.dict_of(DICT_LEN)
    return _compress(ref, O, corpus, lambda v, cap: ref_compress(rd, d, v, cap), _common("compress_dict", dictionary="@dic"),
                     setup=_with_dictionary, teardown=_close_dictionary)


_HC_REF = {}


def compress_hc_dict_case(ref, O, corpus, method="compress_hc_dict"):
    from hcdict_common import Ref
    R, d = _HC_REF.setdefault(id(ref), Ref(ref)), F.dict_of(DICT_LEN)
    return _compress(ref, O, corpus, lambda v, cap: R.compress(d, v, HC_LEVEL, cap), _common(method, dictionary="@dic", level=HC_LEVEL),
                     setup=_with_dictionary, teardown=_close_dictionary)


def compress_hc_dict_sync_case(ref, O, corpus):
    return compress_hc_dict_case(ref, O, corpus, "compress_hc_dict_sync")


def valid_streams(ref, O, corpus):
    """[(name, stream, decoded size)] of every block, from the reference compressor"""
    return [(name, ref.compress_fast(y), len(y)) for name, y, _ in blocks(O, corpus)]


def decode_safe_case(ref, O, corpus):
    def x_result(x, it):
        r, by = ref.decompress_safe_raw(x, it[3])
        return r, by[:r] if r >= 0 else None, 0
    items = F.decode_safe_items(ref, valid_streams(ref, O, corpus))
    return _block_case(items, [flipped(it[1]) for it in items], x_result, _common("decompress_safe"))


def decode_fast_case(ref, O, corpus):
    def x_result(x, it):
        r, by = O.decompress_fast_bounded(x, len(x), it[3])
        return r, by if r >= 0 else None, 0
    items = F.decode_fast_items(O, valid_streams(ref, O, corpus))
    return _block_case(items, [flipped(it[1]) for it in items], x_result, _common("decompress_fast"))


def decode_partial_case(ref, O, corpus):
    """targets of 1, 4096 and the whole block in turn; p1 = target, p2 = capacity; the slot owns min(target, capacity) bytes"""
    from partial_common import ref_partial
    run = ref_partial(ref)

    def x_result(x, it):
        r, by = run(x, it[3], it[6])
        return r, by if r >= 0 else None, 0

    def call(amd, t):
        amd.DeviceBatch.decompress_safe_partial(t["src"], t["src_off"], t["src_len"], t["dst"], t["dst_off"], t["p1"], t["cap"], t["out"])
    items = F.decode_partial_items(ref, valid_streams(ref, O, corpus), targets=lambda k, cap: ((1, 4096, cap)[k % 3],))
    return _block_case(items, [flipped(it[1]) for it in items], x_result, call, p2_in="cap")


def decode_size_case(ref, O, corpus):
    from size_common import ref_size
    run = ref_size(ref)

    def call(amd, t):
        amd.DeviceBatch.decoded_size(t["src"], t["src_off"], t["src_len"], t["p1"], t["out"])
    items = F.decode_size_items(ref, valid_streams(ref, O, corpus))
    return _block_case(items, [flipped(it[1]) for it in items], lambda x, it: (run(x, it[3]), None, 0), call, has_dst=False)


def decode_dict_case(ref, O, corpus):
    """every block (but the empty ones) compressed against the dictionary by the reference's two dictionary compressors in turn"""
    from dict_common import RefDict
    rd, d = RefDict(ref), F.dict_of(DICT_LEN)
    valid = [(name, rd.compress(d, y, HC_LEVEL if k & 1 else 0), len(y)) for k, (name, y, _) in enumerate(blocks(O, corpus)) if y]

    def x_result(x, it):
        r, by = rd.decode(x, it[3], d)
        return r, by if r >= 0 else None, 0

    def setup(amd, torch, dev):
        return {"d_dev": torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev)}
    items = F.decode_dict_items(rd, d, valid)
    return _block_case(items, [flipped(it[1]) for it in items], x_result, _common("decompress_safe_dict", dictionary="@d_dev"), setup=setup)


def _xxh_case(ref, O, corpus, bits):
    fn = ref.xxh32 if bits == 32 else ref.xxh64
    seed = 0x9747b28c
    lay = Layout()
    blks = blocks(O, corpus)
    off = [lay.source(y, x) for _, y, x in blks]
    src_y, src_x = lay.tail()
    n = len(blks)

    def call(amd, t):
        getattr(amd.DeviceBatch, "xxh%d" % bits)(t["src"], t["src_off"], t["src_len"], seed, t["out"])
    ins = {"src_off": ("int64", off, [0] * n), "src_len": ("int32", [len(y) for _, y, _ in blks], [0] * n)}
    outs = {"out": ("uint%d" % bits, [fn(y, seed) for _, y, _ in blks], [fn(x, seed) for _, _, x in blks])}
    return Case(src_y, src_x, ins, 0, [], outs, call)


def xxh32_case(ref, O, corpus):
    return _xxh_case(ref, O, corpus, 32)


def xxh64_case(ref, O, corpus):
    return _xxh_case(ref, O, corpus, 64)


def xxh_stream_case(ref, O, corpus):
    """one handle: reset, then the source in two pieces.  The digest is fetched on the host once the stream is done"""
    b = corpus["book1[:200000]"]
    y, x = b"\x33" + b[:70001], b"\xCC" + b[100001:170002]
    cut = 33333
    seed = 0x9747b28c

    def setup(amd, torch, dev):
        return {"hash": amd.StreamingXXHash32(seed)}

    def call(amd, t):
        import torch
        st = torch.cuda.current_stream(t["src"].device).cuda_stream
        t["hash"].reset()
        t["hash"].update_device(t["src"].data_ptr() + 1, cut, stream=st)
        t["hash"].update_device(t["src"].data_ptr() + 1 + cut, len(y) - 1 - cut, stream=st)
    return Case(y, x, {}, 0, [], {"digest": ("uint32", [ref.xxh32(y[1:], seed)], [ref.xxh32(x[1:], seed)])}, call, setup,
                lambda t: t["hash"].close(), lambda amd, t: {"digest": [t["hash"].getValue()]})


def gen_blocks_case(ref, O, corpus):
    """no source: GEN_BLOCKS App. F blocks of GEN_LEN bytes, GUARD bytes apart"""
    stride = GEN_LEN + GUARD

    def call(amd, t):
        amd.DeviceBatch.gen_blocks(t["dst"][GUARD:], stride, GEN_LEN, GEN_BLOCKS, first_idx=GEN_FIRST)
    slots = [Slot("block %d" % i, GUARD + i * stride, GEN_LEN, O.gen_block(GEN_LEN, GEN_FIRST + i), None) for i in range(GEN_BLOCKS)]
    return Case(b"", b"", {}, GUARD + GEN_BLOCKS * stride, slots, {}, call)


def container_want(ref, kind, data, blk):
    """what the reference writers emit for `data` cut into blocks of blk bytes (LZ4FrameOutputStream.writeBlock with block checksums /
    LZ4BlockOutputStream.flushBufferedData)"""
    out = bytearray()
    for o in range(0, len(data), blk):
        v = data[o:o + blk]
        c = ref.compress_fast(v)
        raw = len(c) >= len(v)
        pay = v if raw else c
        if kind == 0:
            out += (len(pay) | (0x80000000 if raw else 0)).to_bytes(4, "little") + pay + ref.xxh32(pay, 0).to_bytes(4, "little")
        else:
            out += (b"LZ4Block" + bytes([(0x10 if raw else 0x20) | 12]) + len(pay).to_bytes(4, "little") + len(v).to_bytes(4, "little")
                    + (ref.xxh32(v, 0x9747b28c) & 0x0FFFFFFF).to_bytes(4, "little") + pay)
    return bytes(out)


def _container_data(O, corpus):
    """40 blocks of CONTAINER_BLOCK bytes: text, App. F and random bytes (stored raw) -> (y, x)"""
    b = corpus["book1[:200000]"]
    n = CONTAINER_BLOCK
    y = b[:16 * n] + O.gen_block(16 * n, 3) + random.Random(60).randbytes(8 * n)
    x = b[100001:100001 + 16 * n] + O.gen_block(16 * n, 103) + random.Random(160).randbytes(8 * n)
    return y, x


def container_blocks_case(ref, O, corpus, kind=0):
    """the whole container is one slot of exactly the reference's size: nothing may be written behind the total"""
    y, x = _container_data(O, corpus)
    want, want_x = container_want(ref, kind, y, CONTAINER_BLOCK), container_want(ref, kind, x, CONTAINER_BLOCK)
    cap = len(y) + 64 * (len(y) // CONTAINER_BLOCK)
    assert max(len(want), len(want_x)) <= cap

    def call(amd, t):
        amd.DeviceBatch.container_blocks(kind, t["src"][1:1 + len(y)], CONTAINER_BLOCK, t["dst"][GUARD:GUARD + cap], t["total"], block_checksum=(kind == 0))
    return Case(b"\x33" + y, b"\xCC" + x, {}, GUARD + cap + GUARD, [Slot("container", GUARD, len(want), want, want_x[:len(want)])],
                {"total": ("int64", [len(want)], [len(want_x)])}, call)


def container_decode_case(ref, O, corpus, kind=1):
    """the reference's container of Y, read back: block k decodes to its slot of CONTAINER_BLOCK bytes, GUARD bytes between the slots.
    The decoy is the container of X cut or padded to the same length"""
    y, x = _container_data(O, corpus)
    body = container_want(ref, kind, y, CONTAINER_BLOCK)
    body_x = (container_want(ref, kind, x, CONTAINER_BLOCK) + bytes(len(body)))[:len(body)]
    n = len(y) // CONTAINER_BLOCK
    slot = CONTAINER_BLOCK + GUARD

    def setup(amd, torch, dev):
        wsb = amd.lib().lz4hip_container_decode_workspace_bytes(n)
        return {"ws": torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev), "wsb": wsb}

    def call(amd, t):
        import torch
        rc = amd.lib().lz4hip_container_decode_dev(kind, 1 if kind == 0 else 0, t["src"].data_ptr() + 1, len(body), CONTAINER_BLOCK,
                                                   t["dst"].data_ptr() + GUARD, slot, n, t["sizes"].data_ptr(), t["info"].data_ptr(), t["ws"].data_ptr(),
                                                   t["wsb"], 0, torch.cuda.current_stream(t["src"].device).cuda_stream)
        assert rc == 0, amd.lib().lz4hip_last_error()
    slots = [Slot("block %d" % k, GUARD + k * slot, CONTAINER_BLOCK, y[k * CONTAINER_BLOCK:(k + 1) * CONTAINER_BLOCK],
                  x[k * CONTAINER_BLOCK:(k + 1) * CONTAINER_BLOCK]) for k in range(n)]
    # info[4] (liblz4's code when a decode failed) is 0 on a clean run; the decoy's values are not known block by block: None
    outs = {"sizes": ("int32", [CONTAINER_BLOCK] * n, None), "info": ("int64", [n, len(body), 1, len(y), 0], None)}
    return Case(b"\x33" + body + bytes(64), b"\xCC" + body_x + bytes(64), {}, GUARD + n * slot, slots, outs, call, setup)


CHAIN_SIZES = ([1000] * 6, [4096] * 3, [65536, 4096], [100] * 20, [5, 0, 13, 300, 12, 2000], [70000], [64, 1, 12])


def _chains(history):
    """the same block sizes over two stretches of book1: -> (chains of Y, chains of X)"""
    from cchain_common import book1, chain_of
    b = book1()
    ys, xs, o = [], [], 1000
    for k, sizes in enumerate(CHAIN_SIZES):
        n, P = sum(sizes), (0, 100, 7)[k % 3] if history else 0
        ys.append(chain_of("chain %d" % k, b[o:o + n], sizes, history=b[o - P:o]))
        xs.append(chain_of("decoy %d" % k, b[300000 + o:300000 + o + n], sizes, history=b[300000 + o - P:300000 + o]))
        o += n + 500
    return ys, xs


def compress_chain_case(ref, O, corpus):
    """cchain_common's layout of one call (CPacked: 64 guard bytes of 0xA5) and its check against the reference's stream compressor"""
    from cchain_common import CPacked, RefCChain, expected
    rc = RefCChain(ref)
    ys, xs = _chains(True)
    pk, pkx = CPacked(ys, fill=FILL), CPacked(xs, fill=FILL)
    assert (pk.chain_src_off, pk.src_len, pk.dst_off, len(pk.src)) == (pkx.chain_src_off, pkx.src_len, pkx.dst_off, len(pkx.src))
    want, want_x = expected(rc, ys), expected(rc, xs)
    nb, nc = pk.n_blocks, pk.n_chains

    def call(amd, t):
        amd.DeviceBatch.compress_fast_chain(t["src"], t["chain_src_off"], t["src_len"], t["chain_first"], t["dst"], t["dst_off"], t["dst_cap"],
                                            t["out"], t["consumed"], t["prefix"])
    ins = {"chain_src_off": ("int64", pk.chain_src_off, pk.chain_src_off), "src_len": ("int32", pk.src_len, [0] * nb),
           "chain_first": ("int32", pk.chain_first, pk.chain_first), "dst_off": ("int64", pk.dst_off, pk.dst_off),
           "dst_cap": ("int32", pk.dst_cap, [0] * nb), "prefix": ("int32", pk.prefix, [0] * nc)}
    outs = {"out": ("int32", [r for w in want for r in w[0]], [r for w in want_x for r in w[0]]),
            "consumed": ("int64", [w[1] for w in want], [w[1] for w in want_x])}
    slots = [Slot("%s block %d" % (ch.name, i), pk.dst_off[pk.chain_first[c] + i], pk.dst_cap[pk.chain_first[c] + i], want[c][2][i], want_x[c][2][i],
                  len(ch.blocks[i][0]))
             for c, ch in enumerate(ys) for i in range(len(ch.blocks))]
    return Case(pk.src, pkx.src, ins, len(pk.dst), slots, outs, call, check=lambda dst, got: pk.check(dst, got["out"], got["consumed"], want))


def decode_chain_case(ref, O, corpus):
    """the reference's linked streams of chains without history, decoded chain by chain into regions with GUARD bytes around them"""
    from cchain_common import RefCChain
    rc = RefCChain(ref)
    ys, _ = _chains(False)
    lay = Layout()
    src_off, src_len, dst_cap, first, cdo, ccap, slots = [], [], [], [0], [], [], []
    for ch in ys:
        outs, done, by = rc.compress(ch)
        assert done == len(ch.data) and all(r == len(s) > 0 for r, s in zip(outs, by))
        sizes = [len(s) for s, _ in ch.blocks]
        data = rc.decode(b"", by, sizes)
        assert data == ch.data
        for s, n in zip(by, sizes):
            src_off.append(lay.source(s, flipped(s))); src_len.append(len(s)); dst_cap.append(n)
        first.append(len(src_off))
        at = lay.slot(len(data))
        cdo.append(at); ccap.append(len(data))
        slots.append(Slot(ch.name, at, len(data), data, None))
    src_y, src_x = lay.tail()
    nb, nc = len(src_off), len(ys)

    def call(amd, t):
        amd.DeviceBatch.decompress_safe_chain(t["src"], t["src_off"], t["src_len"], t["dst_cap"], t["chain_first"], t["dst"], t["chain_dst_off"],
                                              t["chain_dst_cap"], t["out"], t["chain_out"])
    ins = {"src_off": ("int64", src_off, [0] * nb), "src_len": ("int32", src_len, [0] * nb), "dst_cap": ("int32", dst_cap, [0] * nb),
           "chain_first": ("int32", first, first), "chain_dst_off": ("int64", cdo, cdo), "chain_dst_cap": ("int64", ccap, [0] * nc)}
    # the decoy: no flipped first block of a chain decodes (asserted in test_userstream_table.py), so no chain gives Y's values
    outs = {"out": ("int32", dst_cap, None), "chain_out": ("int64", ccap, None)}
    return Case(src_y, src_x, ins, lay.dst_len, slots, outs, call)


# ---- the pieces of the tests that are not one small call per entry point -------------------------------------------------------------
def sampled_blocks(n):
    """the 32 blocks whose streams decode_route_kernel (csrc/decode.hip) samples in a launch of n blocks: wavefront w of its 16 looks at
    blocks ((2 w + k) n) / 32 + n / 64 for k = 0, 1 -- provided the stream has 4 KiB or more"""
    return [min(((2 * w + k) * n) // 32 + n // 64, n - 1) for w in range(16) for k in (0, 1)]


def routed_case(ref, O, corpus, kind, fast, n):
    """a decode launch that is routed on the device (n > 16 blocks per CU): blocks of 64 .. 1000 bytes, the sampled ones of 16 KiB
    (streams of 4 KiB and more: the sampler has something to read); text slices or App. F blocks; the safe or the fast decoder"""
    from dict_common import book1
    b = book1()
    big = set(sampled_blocks(n))
    size = lambda i: 16384 if i in big else 64 + (i * 37) % 937
    vs = [b[(173 * i) % (len(b) - 16384):][:size(i)] if kind == "text" else O.gen_block(size(i), i) for i in range(n)]
    valid = [("%s %d" % (kind, i), ref.compress_fast(v), len(v)) for i, v in enumerate(vs)]
    assert all(len(valid[i][1]) >= 4096 for i in big)
    items = F.decode_fast_items(O, valid) if fast else F.decode_safe_items(ref, valid)
    return _block_case(items, [it[1] for it in items], None, _common("decompress_fast" if fast else "decompress_safe"))


XXH_STEPS = (1, 2, 3, 5, 11, 15, 16, 17, 31, 32, 33, 63, 64, 1000, 4096, 8192, 50000)     # test_gpu_xxhash.py::test_streaming_equals_one_shot


def xxh_pieces(n, seed):
    """[(offset, length)]: n bytes cut into pieces of the split sizes of test_streaming_equals_one_shot"""
    rng = random.Random(seed)
    out, pos = [], 0
    while pos < n:
        step = min(n - pos, rng.choice(XXH_STEPS))
        out.append((pos, step))
        pos += step
    return out


def check(case, dst, got):
    """a call's destination bytes and result arrays (as the snapshots hold them) against the reference -> [problems]: the values, the
    bytes of every slot, and every byte outside the slots' results still FILL"""
    bad = []
    for name, (dtype, want, _) in case.outs.items():
        mask = (1 << int(dtype[4:])) - 1 if dtype.startswith("uint") else -1      # (a uint array is fetched as the int of its width)
        have = [int(v) & mask for v in got[name]]
        if have != [int(v) for v in want]:
            k = next((i for i, (a, b) in enumerate(zip(have, want)) if a != int(b)), None)
            bad.append((name, "values differ, first at", k, None if k is None else (have[k], int(want[k]))))
    if case.check:
        return bad + case.check(dst, got)
    if not case.dst_len:
        return bad
    dst = bytes(dst)
    assert len(dst) == case.dst_len
    rest = bytearray(dst)
    for s in case.slots:
        if s.out is not None and dst[s.at:s.at + len(s.out)] != s.out:
            what = "the decoy's bytes" if s.x_out and dst[s.at:s.at + len(s.x_out)] == s.x_out else \
                   "nothing written" if dst[s.at:s.at + len(s.out)] == bytes([FILL]) * len(s.out) else "bytes differ"
            bad.append((s.name, what, s.at))
        rest[s.at:s.at + s.own] = bytes([FILL]) * s.own
    if bytes(rest) != bytes([FILL]) * case.dst_len:
        k = next(i for i, v in enumerate(rest) if v != FILL)
        bad.append(("bytes written outside the slots, first at", k))
    return bad


def decoy_differs(case):
    """what the decoy must be good for -> [problems]: the reference's result for X differs from its result for Y in every block whose
    bytes are compared (a block without input bytes has nothing to differ in), and X has Y's length"""
    bad = []
    if len(case.src_x) != len(case.src_y):
        bad.append(("the decoy's length", len(case.src_x), len(case.src_y)))
    if case.src_y and case.src_x == case.src_y:
        bad.append("the decoy is the input")
    for s in case.slots:
        if s.src_n and s.out and len(s.out) > 1 and s.x_out is not None and s.x_out[:len(s.out)] == s.out:      # (one byte: the token of an empty block)
            bad.append((s.name, "the decoy gives the same bytes"))
    for name, (_, want, want_x) in case.outs.items():
        if want_x is not None and not case.slots:
            same = [k for k, (a, b) in enumerate(zip(want, want_x)) if a == b]
            if len(same) > len(want) // 8:          # (the empty blocks)
                bad.append((name, "the decoy gives the same values at", same[:8]))
    return bad


class Entry(NamedTuple):
    call: str              # the DeviceBatch method, lib() function or class method that reaches the entry point
    cases: str             # the case builder of this module
    expected: str          # where the expected values come from
    syncs: bool            # the header says that the call waits for its stream, every time
    first_syncs: bool = False   # ... that the first call of a dictionary handle on a device does (the tests make it in a warm-up)
    own_scratch: bool = True    # the library allocates the call's scratch itself (False: the caller's workspace)


TABLE = {
    "lz4hip_compress_fast_batch_dev": Entry("DeviceBatch.compress_fast", "compress_fast_case", "ref.compress_fast_raw", False),
    "lz4hip_compress_fast_accel_batch_dev": Entry("DeviceBatch.compress_fast(acceleration)", "compress_accel_case", "RefMore.accel", False),
    "lz4hip_compress_dest_size_batch_dev": Entry("DeviceBatch.compress_dest_size", "dest_size_case", "RefMore.dest_size", False),
    "lz4hip_compress_hc_batch_dev_ws": Entry("DeviceBatch.compress_hc", "compress_hc_case", "ref.compress_hc_raw", False, own_scratch=False),
    "lz4hip_compress_hc_batch_dev": Entry("DeviceBatch.compress_hc_sync", "compress_hc_sync_case", "ref.compress_hc_raw", True),
    "lz4hip_compress_hc_dest_size_batch_dev_ws": Entry("DeviceBatch.compress_hc_dest_size", "hc_dest_size_case", "RefMore.hc_dest_size", False,
                                                       own_scratch=False),
    "lz4hip_compress_hc_dest_size_batch_dev": Entry("DeviceBatch.compress_hc_dest_size_sync", "hc_dest_size_sync_case", "RefMore.hc_dest_size", True),
    "lz4hip_compress_fast_dict_batch_dev": Entry("DeviceBatch.compress_dict", "compress_dict_case", "dictc_common.ref_compress", False, first_syncs=True),
    "lz4hip_compress_hc_dict_batch_dev_ws": Entry("DeviceBatch.compress_hc_dict", "compress_hc_dict_case", "hcdict_common.Ref", False, first_syncs=True,
                                                  own_scratch=False),
    "lz4hip_compress_hc_dict_batch_dev": Entry("DeviceBatch.compress_hc_dict_sync", "compress_hc_dict_sync_case", "hcdict_common.Ref", True),
    "lz4hip_decompress_safe_dict_batch_dev": Entry("DeviceBatch.decompress_safe_dict", "decode_dict_case", "dict_common.RefDict.decode", False),
    "lz4hip_decompress_safe_batch_dev": Entry("DeviceBatch.decompress_safe", "decode_safe_case", "ref.decompress_safe_raw", False),
    "lz4hip_decompress_fast_batch_dev": Entry("DeviceBatch.decompress_fast", "decode_fast_case", "O.decompress_fast_bounded", False),
    "lz4hip_decompress_safe_partial_batch_dev": Entry("DeviceBatch.decompress_safe_partial", "decode_partial_case", "partial_common.ref_partial", False),
    "lz4hip_decompressed_size_batch_dev": Entry("DeviceBatch.decoded_size", "decode_size_case", "size_common.ref_size", False),
    "lz4hip_xxh32_batch_dev": Entry("DeviceBatch.xxh32", "xxh32_case", "ref.xxh32", False),
    "lz4hip_xxh64_batch_dev": Entry("DeviceBatch.xxh64", "xxh64_case", "ref.xxh64", False),
    "lz4hip_xxh_stream_update_dev": Entry("StreamingXXHash32.update_device", "xxh_stream_case", "ref.xxh32", False),
    "lz4hip_gen_blocks_dev": Entry("DeviceBatch.gen_blocks", "gen_blocks_case", "O.gen_block", False),
    "lz4hip_container_blocks_dev": Entry("DeviceBatch.container_blocks", "container_blocks_case", "ref.compress_fast, ref.xxh32", False, own_scratch=False),
    "lz4hip_container_decode_dev": Entry("lib().lz4hip_container_decode_dev", "container_decode_case", "ref.compress_fast, ref.xxh32", False,
                                         own_scratch=False),
    "lz4hip_decompress_safe_chain_batch_dev": Entry("DeviceBatch.decompress_safe_chain", "decode_chain_case", "cchain_common.RefCChain", False),
    "lz4hip_compress_fast_chain_batch_dev": Entry("DeviceBatch.compress_fast_chain", "compress_chain_case", "cchain_common.RefCChain", False),
}
EXEMPT = {
    "lz4hip_dbg_compress_fast_profile_dev": "developer diagnostic, not in the release library",
}
SOURCES = ("ref.", "RefMore.", "dictc_common.", "hcdict_common.", "dict_common.", "partial_common.", "size_common.", "cchain_common.",
           "O.decompress_fast_bounded", "O.gen_block")


_CASES = {}


def case_of(fn, ref, O, corpus):
    """the entry point's case, built once (the reference runs once per entry; nothing changes a Case afterwards)"""
    if fn not in _CASES:
        _CASES[fn] = globals()[TABLE[fn].cases](ref, O, corpus)
    return _CASES[fn]


# ---- what the header says about an entry point's synchronisation ---------------------------------------------------------------------
GENERAL = ("work is enqueued on `stream`", "returns without synchronising", "every other *_dev entry never synchronises")


def header_says(fn, text):
    """-> (syncs, first_syncs) from the comments of include/lz4hip.h that describe `fn`: a comment directly in front of a *_dev
    declaration describes that function; any other comment describes the functions it names.  Where such a comment tells a plain form
    from "the _ws form", a function whose name ends in _ws is described by the part from there on of its plain form's comments; every
    other function by the part in front"""
    ws = fn.endswith("_ws")
    plain = fn[:-3] if ws else fn
    about = []
    for m in re.finditer(r"/\*.*?\*/", text, flags=re.S):
        c = m.group(0)
        owner = re.match(r"\s*int (lz4hip_\w*_dev\w*)\s*\(", text[m.end():])
        if (owner.group(1) == plain) if owner else re.search(r"\b%s\b" % re.escape(plain), c):
            cut = c.find("_ws form")
            if cut >= 0 or not ws:          # (a comment of the plain form that does not speak of the _ws form says nothing about it)
                about.append(c if cut < 0 else c[cut:] if ws else c[:cut])
    # (no comment of its own: the section's sentence holds -- "returns without synchronising", GENERAL below)
    said = " ".join(" ".join(about).split())
    return bool(re.search(r"synchronises `stream`", said)), bool(re.search(r"waits for `stream` once", said))
