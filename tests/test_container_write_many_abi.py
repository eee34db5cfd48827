"""No-GPU checks of the many-container write call: the two C-ABI entry points are declared, exported and bound; every argument error is
said, with its message, before a device is looked for; the call of no items is fine; a well-formed call fails LOUDLY without a device;
the bound call equals the plain arithmetic on the case list; the header's section says what the call promises and leaves out."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import container_write_many_common as wm
from conftest import ROOT
from support import E_ARG, E_NO_DEVICE, no_device

NEW = ("lz4hip_container_blocks_many_bound", "lz4hip_container_blocks_many")


def test_write_many_symbols_declared_exported_and_bound(amd):
    h = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    so = os.path.join(ROOT, "lz4-java_amd", "liblz4hip.so")
    exported = set(re.findall(r" T (lz4hip_\w+)", subprocess.check_output(["nm", "-D", so]).decode()))
    for s in NEW:
        assert s in exported and s in amd.C_ABI and hasattr(amd.lib(), s), s
    assert re.search(r"int lz4hip_container_blocks_many_bound\(int kind, const uint64_t\* src_len, const uint32_t\* block_size, const uint8_t\* flags,\s*"
                     r"const uint32_t\* gap_head, const uint32_t\* gap_tail, uint32_t n_items, uint32_t\* item_blocks,\s*uint64_t\* item_dst_bytes\);", h)
    assert re.search(r"int lz4hip_container_blocks_many\(int kind, int level, const uint8_t\* src, const uint64_t\* src_off, const uint64_t\* src_len,\s*"
                     r"const uint32_t\* block_size, const uint8_t\* flags, const uint32_t\* gap_head, const uint32_t\* gap_tail,\s*"
                     r"uint32_t n_items, uint8_t\* dst, uint64_t dst_cap, uint64_t\* item_dst_off, uint32_t\* content_hash\);", h)
    u64p, u32p, u8p = (C.POINTER(t) for t in (C.c_uint64, C.c_uint32, C.c_uint8))
    assert amd.C_ABI[NEW[0]] == (C.c_int, [C.c_int, u64p, u32p, u8p, u32p, u32p, C.c_uint32, u32p, u64p])
    assert amd.C_ABI[NEW[1]] == (C.c_int, [C.c_int, C.c_int, C.c_void_p, u64p, u64p, u32p, u8p, u32p, u32p, C.c_uint32, u8p, C.c_uint64, u64p, u32p])
    strings = subprocess.check_output(["strings", so]).decode(errors="replace")
    for k in ("container_layout_many_kernel", "container_scan_many_kernel", "container_copy_many_kernel"):
        assert k in strings, k
    assert callable(amd.LZ4HIPBatch.containerBlocksMany)
    S = __import__("importlib").import_module("lz4-java_amd.streams")
    assert callable(S.HIPEngine.containerBlocksMany) and callable(S.writeFrames) and callable(S.writeBlockStreams)


def test_write_many_header_section(amd):
    h = " ".join(open(os.path.join(ROOT, "include", "lz4hip.h")).read().replace("*", " ").split())
    for sentence in ("The contract is the existing call, item by item",
                     "items may lie anywhere in src, in any order, and may overlap",
                     "content_hash[c] is 0 where bit 1 is clear",
                     "they come back as zeros",
                     "An item of 0 bytes has no blocks and contributes only its gaps",
                     "nothing at or behind dst + item_dst_off[n_items] is written",
                     "LZ4HIP_E_ARG is said before a device is looked for",
                     "n_items == 0 is LZ4HIP_OK with item_dst_off[0] = 0",
                     "The call runs on the engine's first device",
                     "An item of millions of blocks belongs to lz4hip_container_blocks",
                     "Out of scope: device-pointer forms; mixing kinds in one call; sharding items over several devices; linked-block frames."):
        assert sentence in h, sentence


def _items():
    return [("a", b"x" * 3000, 1000, True, 7, 19, True), ("b", b"y" * 70, 64, False, 0, 0, False)]


def _call(L, kind, level, pk, dst_cap, null=None):
    n = pk.n
    dst = np.zeros(min(max(dst_cap, 1), 1 << 16), np.uint8)   # (a call with a larger dst_cap here ends in an argument error: dst is not touched)
    doff, hashes = np.full(n + 1, 9, np.uint64), np.zeros(n + 1, np.uint32)
    args = list(pk.head(kind, level)) + [wm._p(dst, C.c_uint8), dst_cap, wm._p(doff, C.c_uint64), wm._p(hashes, C.c_uint32)]
    if null is not None:
        args[null] = None
    return L.lz4hip_container_blocks_many(*args), doff


def _bound(L, kind, pk, null=None):
    nb, need = np.zeros(pk.n + 1, np.uint32), np.zeros(pk.n + 1, np.uint64)
    args = list(pk.bound_args(kind)) + [wm._p(nb, C.c_uint32), wm._p(need, C.c_uint64)]
    if null is not None:
        args[null] = None
    return L.lz4hip_container_blocks_many_bound(*args)


def test_write_many_argument_errors_come_before_the_device_check(amd):
    """every LZ4HIP_E_ARG case with its message, on a machine without a device too: it is said before a device is looked for"""
    L = amd.lib()
    err = L.lz4hip_last_error
    pk = wm.Packed(_items())
    nb, need = wm.bound_many(L, 0, pk)
    assert list(nb) == [3, 2] and list(need) == [7 + 3000 + 3 * 8 + 19, 70 + 2 * 4]
    cap = int(need.sum())
    good = _call(L, 0, 0, pk, cap)[0]
    assert good == (E_NO_DEVICE if no_device() else 0), (good, err())
    if no_device():
        assert b"no HIP device" in err()
    for kind in (-1, 2):
        assert _call(L, kind, 0, pk, cap)[0] == E_ARG and b"kind" in err()
        assert _bound(L, kind, pk) == E_ARG and b"kind" in err()
    for k in (2, 3, 4, 5, 6, 10, 12):                  # src, src_off, src_len, block_size, flags, dst, item_dst_off
        assert _call(L, 0, 0, pk, cap, null=k)[0] == E_ARG and b"null pointer" in err(), k
    for k in (1, 2, 3, 7, 8):                          # src_len, block_size, flags, item_blocks, item_dst_bytes
        assert _bound(L, 0, pk, null=k) == E_ARG and b"null pointer" in err(), k
    assert _call(L, 0, 0, pk, cap, null=7)[0] == good and _call(L, 0, 0, pk, cap - 7, null=7)[0] == good       # gap_head NULL: 0 for every item
    assert _call(L, 0, 0, pk, cap - 19, null=8)[0] == good and _bound(L, 0, pk, null=4) == 0 and _bound(L, 0, pk, null=5) == 0
    for bs in (0, 63, (32 << 20) + 1, 0xFFFFFFFF):
        bad = wm.Packed(_items()); bad.bs[1] = bs
        assert _call(L, 0, 0, bad, cap)[0] == E_ARG and b"block size must be 64 .. 32 MiB" in err(), bs
        assert _bound(L, 0, bad) == E_ARG and b"block size must be 64 .. 32 MiB" in err(), bs
    bad = wm.Packed(_items()); bad.len[1] = 1 << 31
    assert _call(L, 0, 0, bad, 1 << 40)[0] == E_ARG and b"src_len must be at most 2^31 - 1" in err()
    assert _bound(L, 0, bad) == E_ARG and b"src_len must be at most 2^31 - 1" in err()
    for fl in (4, 8, 0x80, 0x83):
        bad = wm.Packed(_items()); bad.fl[0] = fl
        assert _call(L, 0, 0, bad, cap)[0] == E_ARG and b"only bit 0 (block checksums) and bit 1 (content hash) are defined" in err(), fl
        assert _bound(L, 0, bad) == E_ARG
    assert _call(L, 1, 0, pk, cap + 100)[0] == E_ARG and b"belongs to kind 0" in err()          # bit 0 with kind 1
    assert _bound(L, 1, pk) == E_ARG and b"belongs to kind 0" in err()
    assert _call(L, 0, 0, pk, cap, null=13)[0] == E_ARG and b"content_hash is NULL" in err()      # bit 1 without content_hash
    nohash = wm.Packed([it[:6] + (False,) for it in _items()])
    assert _call(L, 0, 0, nohash, cap, null=13)[0] == good                                          # ... which may be NULL when nobody asks
    assert _call(L, 0, 0, pk, cap - 1)[0] == E_ARG and b"dst_cap is below the sum of item_dst_bytes" in err()
    # more than 2^31 - 1 - n_items blocks in all: 65 items of 2^31 - 1 bytes in blocks of 64 (the arrays are small; no source is touched)
    many = wm.Packed([("z", b"", 64, False, 0, 0, False)] * 65)
    many.len[:65] = 2 ** 31 - 1
    assert _call(L, 0, 0, many, 1 << 50)[0] == E_ARG and b"more than 2^31 - 1 - n_items blocks" in err()
    # more than 2^31 - 1 items: said before any array is read (the arrays here hold one item)
    doff1 = np.full(1, 9, np.uint64)
    assert L.lz4hip_container_blocks_many(0, 0, wm._p(pk.blob, C.c_uint8), wm._p(pk.off, C.c_uint64), wm._p(pk.len, C.c_uint64), wm._p(pk.bs, C.c_uint32),
                                          wm._p(pk.fl, C.c_uint8), None, None, 1 << 31, wm._p(pk.blob, C.c_uint8), 1 << 60, wm._p(doff1, C.c_uint64),
                                          None) == E_ARG and b"more than 2^31 - 1 items" in err()
    # bounds whose sum does not fit 64 bits cannot be built from arrays a test can hold; the check is a guard of the u64 sum alone
    nb, need = wm.bound_many(L, 0, many)
    assert int(nb[0]) == (2 ** 31 - 1 + 63) // 64 and int(need[0]) == 2 ** 31 - 1 + 4 * int(nb[0])


def test_write_many_call_of_no_items(amd):
    L = amd.lib()
    rc, doff = _call(L, 1, 0, wm.Packed([]), 0)
    assert rc == 0 and doff[0] == 0
    doff = np.full(1, 9, np.uint64)
    assert L.lz4hip_container_blocks_many(0, 9, None, None, None, None, None, None, None, 0, None, 0, wm._p(doff, C.c_uint64), None) == 0 and doff[0] == 0
    assert L.lz4hip_container_blocks_many_bound(0, None, None, None, None, None, 0, None, None) == 0
    dst, off, hashes = amd.LZ4HIPBatch.containerBlocksMany(0, [], [])
    assert len(dst) == 0 and list(off) == [0] and len(hashes) == 0
    assert amd.LZ4HIPBatch.containerBlocksManyBound(0, [], []) == []


@pytest.mark.parametrize("kind", [wm.FRAME, wm.LZ4BLOCK])
def test_write_many_bound_equals_the_arithmetic(amd, O, corpus, kind):
    items = wm.for_kind(wm.cases(O, corpus), kind)
    nb, need = wm.bound_many(amd.lib(), kind, wm.Packed(items))
    for c, (name, d, bs, cks, gh, gt, h) in enumerate(items):
        assert (int(nb[c]), int(need[c])) == (wm.item_blocks(len(d), bs), wm.item_bound(kind, len(d), bs, cks, gh, gt)), name
    got = amd.LZ4HIPBatch.containerBlocksManyBound(kind, [len(it[1]) for it in items], [it[2] for it in items], [it[3] for it in items],
                                                   [it[4] for it in items], [it[5] for it in items])
    assert got == [(int(a), int(b)) for a, b in zip(nb, need)]
