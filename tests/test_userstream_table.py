"""The stream-contract table of tests/userstream_common.py, checked without a GPU: it names every device entry point include/lz4hip.h
declares (a new one cannot be added without a case on a caller's stream or a stated exemption), its `syncs` flags say what the header
says, and its case builders make what they promise: expected values that the reference alone produces, a decoy of the same shape
whose result differs, and a check that tells the one from the other."""
import inspect
import os
import re

import pytest

import far_common as F
import userstream_common as U
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "lz4hip.h")


def _device_batch():
    import importlib
    return importlib.import_module("lz4-java_amd")


def missing_entries(table, exempt, header=None):
    declared = F.declared_dev_entry_points(header)
    return [f for f in declared if f not in table and f not in exempt]


def test_every_device_entry_point_is_in_the_table_or_exempt():
    declared = F.declared_dev_entry_points()
    assert len(declared) >= 24 and "lz4hip_xxh_stream_update_dev" in declared
    assert not set(U.TABLE) & set(U.EXEMPT)
    missing = missing_entries(U.TABLE, U.EXEMPT)
    assert not missing, "device entry points without a stream-contract case (tests/userstream_common.py TABLE): %s" % missing
    stale = [f for f in list(U.TABLE) + list(U.EXEMPT) if f not in declared]
    assert not stale, "the table names functions the header does not declare: %s" % stale
    assert list(U.EXEMPT) == ["lz4hip_dbg_compress_fast_profile_dev"] and "lz4hip_xxh_stream_update_dev" in U.TABLE


@pytest.mark.parametrize("fn", sorted(U.TABLE))
def test_a_deleted_entry_is_named(fn):
    """without its entry, the function is what the check above reports"""
    assert missing_entries({k: v for k, v in U.TABLE.items() if k != fn}, U.EXEMPT) == [fn]


def test_a_new_declaration_is_missed(tmp_path):
    text = open(HEADER).read()
    p = tmp_path / "lz4hip.h"
    p.write_text(text.replace("#ifdef LZ4HIP_DEV_TOOLS", "int lz4hip_new_thing_batch_dev(const uint8_t* src, int device, void* stream);\n#ifdef LZ4HIP_DEV_TOOLS", 1))
    assert missing_entries(U.TABLE, U.EXEMPT, str(p)) == ["lz4hip_new_thing_batch_dev"]


@pytest.mark.parametrize("fn", sorted(U.TABLE))
def test_syncs_is_what_the_header_says(fn):
    e = U.TABLE[fn]
    syncs, first = U.header_says(fn, open(HEADER).read())
    assert e.syncs == syncs, (fn, "TABLE says syncs =", e.syncs, "the header's comments say", syncs)
    if not e.syncs:
        assert e.first_syncs == first, (fn, "TABLE says first_syncs =", e.first_syncs, "the header's comments say", first)


def test_the_header_states_the_contract():
    text = " ".join(open(HEADER).read().replace("\n *", " ").split())
    for sentence in U.GENERAL:
        assert sentence in text, sentence


def test_the_flags_the_header_fixes():
    """the three entries that size a workspace from a value they read back, and the two whose handle builds an image at its first call"""
    assert sorted(f for f, e in U.TABLE.items() if e.syncs) == ["lz4hip_compress_hc_batch_dev", "lz4hip_compress_hc_dest_size_batch_dev",
                                                               "lz4hip_compress_hc_dict_batch_dev"]
    assert sorted(f for f, e in U.TABLE.items() if e.first_syncs) == ["lz4hip_compress_fast_dict_batch_dev", "lz4hip_compress_hc_dict_batch_dev_ws"]
    assert sorted(f for f, e in U.TABLE.items() if not e.own_scratch) == sorted(
        [f for f in U.TABLE if f.endswith("_ws")] + ["lz4hip_container_blocks_dev", "lz4hip_container_decode_dev"])


def test_the_header_parser_reads_a_changed_sentence(tmp_path):
    """a sentence about synchronisation added to, or taken from, an entry's comment changes what header_says returns"""
    text = open(HEADER).read()
    assert U.header_says("lz4hip_compress_dest_size_batch_dev", text) == (False, False)
    changed = text.replace("/* compress to a target size (see lz4hip_compress_dest_size_batch), device pointers, asynchronous */",
                           "/* compress to a target size (see lz4hip_compress_dest_size_batch), device pointers; synchronises `stream` once */", 1)
    assert changed != text and U.header_says("lz4hip_compress_dest_size_batch_dev", changed) == (True, False)
    assert U.header_says("lz4hip_compress_hc_batch_dev", text)[0] and not U.header_says("lz4hip_compress_hc_batch_dev_ws", text)[0]
    gone = text.replace("and therefore synchronises `stream`", "and therefore waits").replace("it synchronises `stream` ONCE per call", "it waits per call")
    assert not U.header_says("lz4hip_compress_hc_batch_dev", gone)[0]


def test_every_entry_names_its_call_its_builder_and_a_reference():
    amd = _device_batch()
    for fn, e in U.TABLE.items():
        m = re.fullmatch(r"(DeviceBatch|lib\(\)|StreamingXXHash32)\.(\w+)(?:\((\w+)\))?", e.call)
        assert m, (fn, e.call)
        if m.group(1) == "lib()":
            assert m.group(2) == fn, (fn, e.call)
        else:       # the method passes the entry point's name to the library
            assert fn in inspect.getsource(getattr(getattr(amd, m.group(1)), m.group(2))), (fn, e.call, "this method does not call the entry point")
        body = inspect.getsource(getattr(U, e.cases))
        helper = re.search(r"return (\w+_case|_xxh_case)\(", body)           # (the _sync forms and xxh32 / xxh64 share a builder)
        body += inspect.getsource(getattr(U, helper.group(1))) if helper else ""
        assert m.group(2) in body or (helper and "method" in body), (fn, e.cases, "the builder does not make this call")
        for src in e.expected.split(", "):
            assert src.startswith(U.SOURCES), (fn, src, "not one of the references")


@pytest.fixture(scope="module")
def cases(ref, O, corpus):
    return {fn: U.case_of(fn, ref, O, corpus) for fn in U.TABLE}


def synthesize(case, decoy=False):
    """the destination and the result arrays as a correct call leaves them (or as one that worked on the decoy does)"""
    dst = bytearray([U.FILL]) * case.dst_len
    for s in case.slots:
        by = s.x_out if decoy else s.out
        if by:
            dst[s.at:s.at + min(len(by), s.own)] = by[:s.own]
    got = {name: (x if decoy and x is not None else want) for name, (_, want, x) in case.outs.items()}
    return bytes(dst), got


@pytest.mark.parametrize("fn", sorted(U.TABLE))
def test_case_shape_decoy_and_check(cases, fn):
    c = cases[fn]
    if "src_len" in c.ins:
        n = len(c.ins["src_len"][1])
        assert 30 <= n <= 45, (fn, n)
        lens = set(c.ins["src_len"][1])
        assert len(lens) >= 8 and max(lens) >= 4096, (fn, sorted(lens))
    for name, (dtype, real, decoy) in c.ins.items():
        assert len(real) == len(decoy) and dtype in ("int32", "int64"), (fn, name)
    # the layout: odd places, GUARD bytes of room on both sides of every slot, nothing overlaps
    last = 0
    for s in sorted(c.slots, key=lambda s: s.at):
        assert s.at >= last + U.GUARD and s.at + s.own + U.GUARD <= c.dst_len, (fn, s.name, s.at)
        assert s.out is None or len(s.out) <= s.own, (fn, s.name)
        last = s.at + s.own
    if "src_off" in c.ins and "dst_off" in c.ins:
        assert all(o & 1 for o in c.ins["src_off"][1]) and all(o & 1 for o in c.ins["dst_off"][1]), fn
    assert U.decoy_differs(c) == [], fn
    # the check passes what the reference gives and fails the decoy's result, a missing result and a written guard
    dst, got = synthesize(c)
    assert U.check(c, dst, got) == [], fn
    if c.src_y:
        dx, gx = synthesize(c, decoy=True)
        assert U.check(c, dx, gx) != [], (fn, "the decoy's result passes")
    if c.dst_len:
        assert U.check(c, bytes([U.FILL]) * c.dst_len, got) != [], (fn, "an untouched destination passes")
        k = min(s.at for s in c.slots) - 1
        assert U.check(c, dst[:k] + b"\x00" + dst[k + 1:], got) != [], (fn, "a written guard passes")
    for name, (_, want, _) in c.outs.items():
        assert U.check(c, dst, dict(got, **{name: [U.SENTINEL] * len(want)})) != [], (fn, name, "an unwritten result array passes")


def test_the_decoy_of_a_chain_does_not_decode(cases, ref):
    """decode_chain_case states no values for its decoy: the flipped first block of every chain fails in the reference decoder, so that
    no chain of the decoy gives the values of the real input"""
    c = cases["lz4hip_decompress_safe_chain_batch_dev"]
    first = c.ins["chain_first"][1]
    for k in first[:-1]:
        o, n, cap = c.ins["src_off"][1][k], c.ins["src_len"][1][k], c.ins["dst_cap"][1][k]
        assert c.src_x[o:o + n] == U.flipped(c.src_y[o:o + n])
        assert ref.decompress_safe_raw(c.src_x[o:o + n], cap)[0] != cap, k
