"""The far-offset table of tests/far_common.py, checked without a GPU: it names every device entry point include/lz4hip.h declares (a new
one cannot be added without a far-offset case or a stated exemption), and its case builders place what they promise -- every place
class on both sides, no overlap, everything inside the view, a red zone that covers every sign-extension -- with expected values that
the reference alone produces."""
import ast
import inspect
import os
import re

import pytest

import far_common as F
from conftest import ROOT


def test_every_device_entry_point_is_in_the_table_or_exempt():
    declared = F.declared_dev_entry_points()
    assert len(declared) >= 24 and "lz4hip_compress_fast_batch_dev" in declared and "lz4hip_compress_hc_dict_batch_dev_ws" in declared
    assert not set(F.TABLE) & set(F.EXEMPT)
    missing = [f for f in declared if f not in F.TABLE and f not in F.EXEMPT]
    assert not missing, "device entry points without a far-offset case (tests/far_common.py TABLE): %s" % missing
    stale = [f for f in list(F.TABLE) + list(F.EXEMPT) if f not in declared]
    assert not stale, "the table names functions the header does not declare: %s" % stale
    assert all(reason for reason in F.EXEMPT.values())


def test_the_header_parser_sees_a_new_entry_point(tmp_path):
    """a declaration added to the header is found, one inside a comment is not"""
    text = open(os.path.join(ROOT, "include", "lz4hip.h")).read()
    p = tmp_path / "lz4hip.h"
    p.write_text(text.replace("#ifdef LZ4HIP_DEV_TOOLS", "/* int lz4hip_commented_dev(void); */\nint lz4hip_new_thing_batch_dev(const uint8_t* src,\n"
                                                          "    const uint64_t* src_off, int device, void* stream);\n#ifdef LZ4HIP_DEV_TOOLS", 1))
    got = F.declared_dev_entry_points(str(p))
    assert "lz4hip_new_thing_batch_dev" in got and "lz4hip_commented_dev" not in got
    assert set(got) - {"lz4hip_new_thing_batch_dev"} == set(F.declared_dev_entry_points())


def test_every_entry_names_a_builder_and_a_test_that_launches_it():
    """the test an entry names exists AND its source holds the entry's call: a new function cannot be listed against a test that
    never launches it"""
    def functions(path):
        text = open(os.path.join(ROOT, "tests", path)).read()
        return {n.name: ast.get_source_segment(text, n) for n in ast.parse(text).body if isinstance(n, ast.FunctionDef)}
    tests, chain_tests = functions("test_gpu_far_offsets.py"), functions("test_gpu_cchain.py")
    for fn, e in F.TABLE.items():
        m = re.fullmatch(r"(?:DeviceBatch|lib\(\))\.(\w+)(?:\((\w+)\))?", e.call)
        assert m, (fn, e.call)
        if e.call.startswith("lib()"):
            assert m.group(1) == fn, (fn, e.call)
        else:       # the DeviceBatch method passes the entry point's name to the library
            src = inspect.getsource(getattr(_device_batch(), m.group(1)))
            assert fn in src, (fn, e.call, "this DeviceBatch method does not call the entry point")
        launched = False
        for t in e.test.split(", "):
            body = chain_tests.get(t.split("::")[1]) if "::" in t else tests.get(t)
            assert body, (fn, t, "no such test")
            launched = launched or (m.group(1) + "(" in body or "." + m.group(1) + "," in body) and (m.group(2) is None or m.group(2) + "=" in body)
        assert launched, (fn, e.call, "none of its tests holds this call")
        for b in e.cases.split(", "):
            assert b.endswith(".py") or hasattr(F, b), (fn, b)
        assert e.expected


def _device_batch():
    import importlib
    return importlib.import_module("lz4-java_amd").DeviceBatch


def test_places():
    assert F.RED == 2 ** 31 + 4096 and F.SPAN == 2 ** 32 + 2 ** 22
    assert F.place_class(F.B31 - 5, 10) == "straddle31" and F.place_class(F.B32 - 1, 2) == "straddle32"
    assert F.place_class(1000, 50) == "control" and F.place_class(F.B32 + 77, 9) == "past32" and F.place_class(F.B31 + 4097, 9) == "behind31"
    assert F.place_class(F.B31 - 10, 10) is None and F.place_class(F.B31, 10) == "behind31"      # touching a boundary is not straddling it
    p = F.Placer(41)
    a, b = p.straddle("straddle32", 100), p.take("straddle32", 100)
    assert F.place_class(a, 100) == "straddle32" and F.place_class(b, 100) == "past32" and b & 1 and b & 127


def _lists(ref, O, corpus):
    """every case list the GPU module launches: (name, slots, has destinations, is a compressor)"""
    yield "compress_fast", F.compress_fast_cases(ref, corpus), True, True
    for a in (2, 64):
        yield "accel %d" % a, F.compress_accel_cases(ref, corpus, a), True, True
    yield "dest_size", F.dest_size_cases(ref, corpus), True, True
    for level in (1, 9, 12):
        yield "hc %d" % level, F.compress_hc_cases(ref, corpus, level), True, True
    for level in (4, 9):
        yield "hc dest_size %d" % level, F.hc_dest_size_cases(ref, corpus, level), True, True
    for L in F.DICT_LENS:
        yield "dict compress %d" % L, F.compress_dict_cases(ref, L), True, True
        yield "dict hc %d" % L, F.compress_hc_dict_cases(ref, L), True, True
        yield "dict decode %d" % L, F.decode_dict_cases(ref, L), True, False
    yield "decode safe", F.decode_safe_cases(ref, O, corpus), True, False
    yield "decode fast", F.decode_fast_cases(ref, O, corpus), True, False
    yield "decode partial", F.decode_partial_cases(ref, O, corpus), True, False
    yield "decode size", F.decode_size_cases(ref, O, corpus), False, False
    yield "xxh long", F.xxh_long_cases(), False, False


@pytest.fixture(scope="module")
def lists(ref, O, corpus):
    return list(_lists(ref, O, corpus))


def test_every_case_list_reaches_every_place_without_overlap(lists):
    for name, slots, has_dst, _ in lists:
        try:
            F.check_layout(slots, need_dst=has_dst)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        # sources and slots are placed independently: a near source with a far slot and the reverse
        if has_dst:
            pairs = {(F.place_class(s.src_at, len(s.data)), F.place_class(s.dst_at, s.own)) for s in slots}
            assert any(a == "control" and b in ("past32", "straddle32") for a, b in pairs), (name, "no near source with a far slot")
            assert any(b == "control" and a in ("past32", "straddle32") for a, b in pairs), (name, "no far source with a near slot")


def test_expected_values_are_the_references_and_not_trivial(lists):
    """every list has results of more than one kind, and its bytes are not all alike; a compressor's list holds blocks that compress,
    blocks that do not fit and the zero result; a decoder's list holds decoded blocks and negative results"""
    for name, slots, has_dst, is_compress in lists:
        if name == "xxh long":
            assert len({len(s.data) for s in slots}) == len(F.XXH_LONG)
            continue
        rets = [s.ret for s in slots]
        assert len(set(rets)) >= 4, (name, "return values", sorted(set(rets)))
        if is_compress:
            assert any(0 < s.ret < len(s.data) for s in slots), (name, "no block that compresses")
            assert any(s.ret > len(s.data) > 0 for s in slots), (name, "no block that expands")
            assert any(s.ret == 0 for s in slots), (name, "no zero result")
            assert any(s.ret == 0 and len(s.data) > 1000 for s in slots), (name, "no block that does not fit")
        else:
            assert any(s.ret < 0 for s in slots) and any(s.ret > 1000 for s in slots), (name, "results", sorted(set(rets))[:6])
        if has_dst:
            outs = [s.out for s in slots if s.out]
            assert len(outs) >= 4 and len(set(outs)) >= 4 and all(len(o) <= s.own for s in slots for o in [s.out] if o is not None), name
            assert all(len(set(o)) > 1 for o in outs if len(o) > 16), (name, "constant expected bytes")


def test_dest_size_lists_check_the_consumed_size(lists):
    for name, slots, _, _ in lists:
        if "dest_size" in name:
            assert any(0 < s.p2 < len(s.data) for s in slots) and any(s.p2 == len(s.data) > 0 for s in slots), name


def test_xxh_short_layout_and_routed_streams(ref, O, corpus):
    img, at, off, lens = F.xxh_short_layout()
    assert len(off) > 512 and at < F.B32 < at + len(img) and min(off) == at and max(o + n for o, n in zip(off, lens)) <= at + len(img)
    assert any(o > F.B32 and o & 1 for o in off) and any(o < F.B32 for o in off)
    assert all(b + 0 >= a + n for (a, n), b in zip(zip(off, lens), off[1:]))
    for kind in ("text", "appf"):
        streams, blocks = F.routed_streams(ref, O, corpus, kind, 64)
        assert len(set(streams)) == 64 and all(ref.decompress_safe(s, 1024) == v for s, v in zip(streams, blocks))
    assert F.GEN_STRIDE * (F.GEN_BLOCKS - 1) > F.B32 and F.GEN_STRIDE * (F.GEN_BLOCKS - 1) + F.GEN_LEN <= F.RED + F.SPAN
    assert F.CONTAINER_BLOCK * F.CONTAINER_BLOCKS > F.B32 and F.CONTAINER_BLOCK * F.CONTAINER_BLOCKS <= F.RED + F.SPAN
