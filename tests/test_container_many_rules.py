"""csrc/container_rules.h on the host, alone: tests/cpp/container_rules_test.cpp is a stand-alone program with the address and
undefined-behaviour sanitizers (never loaded into Python) that walks every body of the case list, each in an allocation of exactly its
length.  Its block table, stop reason and consumed bytes must be those of streams_common.OracleDeviceEngine.containerDecode, which
stands on the reference library: the blocks the oracle delivers are the table's first blocks (their payloads, decoded with the
reference, are the oracle's bytes; their sizes its sizes), and where no block fails its checks the walk's count, stop reason and
position are the oracle's."""
import subprocess

import pytest

import container_many_common as cm
import streams_common as sc
from support import build_sanitized

WALK_REASONS_ONLY = (0, 1, 2, 3, 7)   # END, MORE, TRUNCATED, BLOCK_TOO_BIG, SLOTS: said by the walk alone (6, CORRUPT, by the walk or by a block's checks)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_sanitized("container_rules_test", tmp_path_factory.mktemp("rules"))


def run_walks(exe, tmp_path, items, n_max, slot=2 ** 64 - 1):
    f = tmp_path / ("cases_%d.bin" % n_max)
    f.write_bytes(cm.case_file(items, n_max, slot))
    p = subprocess.run([exe, str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    walks = []
    for line in p.stdout.split("\n"):
        t = line.split()
        if t and t[0] == "C":
            walks.append(dict(blocks=int(t[1]), why=int(t[2]), pos=int(t[3]), dst_bytes=int(t[4]), slot_max=int(t[5]), table=[]))
        elif t:
            walks[-1]["table"].append(dict(zip(("raw", "pay_off", "pay_len", "cap", "stored", "next", "bound"), map(int, t[1:]))))
    assert len(walks) == len(items)
    return walks


@pytest.mark.parametrize("n_max", [1, 2, 64])
def test_rules_walk_equals_the_reference_backed_oracle(exe, tmp_path, ref, O, corpus, n_max):
    case_list = cm.cases(ref, corpus)
    engine = sc.OracleDeviceEngine(ref, O)
    walks = run_walks(exe, tmp_path, case_list, n_max)
    seen = set()
    for (name, kind, body, mb, cks), w in zip(case_list, walks):
        data, sizes, consumed, why, code = engine.containerDecode(kind, body, mb, n_max, cks)
        assert len(w["table"]) == w["blocks"] <= n_max and w["blocks"] >= len(sizes), name
        got = bytearray()
        for k, b in enumerate(w["table"][:len(sizes)]):
            pay = body[b["pay_off"]:b["pay_off"] + b["pay_len"]]
            assert len(pay) == b["pay_len"] and b["next"] == b["pay_off"] + b["pay_len"] + (4 if kind == 0 and cks else 0), (name, k)
            if kind == 0:
                dec = pay if b["raw"] else ref.decompress_safe(pay, b["cap"])
                assert b["cap"] == (b["pay_len"] if b["raw"] else mb) and (not cks or b["stored"] == ref.xxh32(pay, 0)), (name, k)
            else:
                dec = pay if b["raw"] else O.decompress_fast_bounded(pay, len(pay), b["cap"])[1]
                assert b["cap"] == sizes[k] and b["stored"] == (ref.xxh32(dec, cm.CHECK_SEED) & 0x0FFFFFFF), (name, k)
            assert len(dec) == sizes[k], (name, k)
            got += dec
        assert bytes(got) == data, name
        if len(sizes) == w["blocks"] and (why in WALK_REASONS_ONLY or why == 6):
            assert (w["why"], w["pos"]) == (why, consumed), (name, w, why, consumed)      # the walk's own stop
        else:                                                                              # a block failed its checks behind the walk
            assert why in (4, 5, 6) and len(sizes) < w["blocks"], (name, why)
            assert consumed == (w["table"][len(sizes) - 1]["next"] if sizes else 0), name
        assert w["dst_bytes"] == sum(b["bound"] for b in w["table"]) and w["slot_max"] >= max([b["bound"] for b in w["table"]] + [0]), name
        seen.add(why)
    # (the damaged blocks of the case list are second blocks: a walk of one block stops in front of them)
    assert seen >= ({0, 1, 2, 3, 6, 7} if n_max == 1 else {0, 1, 2, 3, 4, 5, 6, 7} if n_max == 2 else {0, 1, 2, 3, 4, 5, 6}), seen


def test_rules_walk_with_small_slots(exe, tmp_path, ref, corpus):
    """slot_bytes, the device walk's argument: a raw frame block or an LZ4Block original length above it stops the walk (reason 3), a
    compressed frame block gets the smaller capacity"""
    text = corpus["book1[:200000]"]
    items = [("f", 0, cm.frame_body(ref, [b"abcd" * 100, __import__("random").Random(1).randbytes(512), text[:100]], False), 65536, False),
             ("b", 1, cm.block_stream(ref, [text[:300], text[:900]], 1024), 1024, False)]
    f, b = run_walks(exe, tmp_path, items, 8, slot=320)
    assert (f["blocks"], f["why"]) == (1, 3) and f["table"][0]["cap"] == 320
    assert (b["blocks"], b["why"]) == (1, 3) and b["table"][0]["cap"] == 300
