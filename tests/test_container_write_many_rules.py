"""csrc/container_write_rules.h on the host, alone: tests/cpp/container_write_rules_test.cpp is a stand-alone program with the address
and undefined-behaviour sanitizers (never loaded into Python) that walks the case list.  Its block tables and bounds must equal a plain
Python restatement, the block of every index must be found in its item through first[], and the container the reference-backed writers
write for an item must be no longer than the item's bound."""
import importlib
import struct
import subprocess

import pytest

import container_write_many_common as wm
from support import build_sanitized


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_sanitized("container_write_rules_test", tmp_path_factory.mktemp("write_rules"))


def run_rules(exe, tmp_path, kind, items):
    f = tmp_path / ("items_%d.bin" % kind)
    f.write_bytes(struct.pack("<II", kind, len(items)) + b"".join(struct.pack("<IIIIQ", bs, fl, gh, gt, n) for (bs, fl, gh, gt, n) in items))
    p = subprocess.run([exe, str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    rows = [line.split() for line in p.stdout.split("\n") if line.split()]
    return [[int(v) for v in r[1:]] for r in rows if r[0] == "I"], [[int(v) for v in r[1:]] for r in rows if r[0] == "B"]


@pytest.mark.parametrize("kind", [wm.FRAME, wm.LZ4BLOCK])
def test_rules_equal_the_plain_restatement_on_the_case_list(exe, tmp_path, ref, O, corpus, kind):
    S = importlib.import_module("lz4-java_amd.streams")
    items = wm.for_kind(wm.cases(O, corpus), kind)
    got_items, got_blocks = run_rules(exe, tmp_path, kind, [(bs, (1 if cks else 0) | (2 if h else 0), gh, gt, len(d)) for (_, d, bs, cks, gh, gt, h) in items])
    assert len(got_items) == len(items)
    want_blocks = []
    written = wm.oracle_items(S, ref, O, corpus, kind, 0)
    for t, ((name, d, bs, cks, gh, gt, h), g) in enumerate(zip(items, got_items)):
        fixed = (8 if cks else 4) if kind == 0 else 21
        slot = (bs + bs // 255 + 16 + 15) & ~15
        biggest = min(bs, len(d))                                     # the item's largest block: what its slots are sized by
        assert g == [wm.item_blocks(len(d), bs), wm.item_bound(kind, len(d), bs, cks, gh, gt), wm.level_nibble(bs), slot, fixed, 4 if kind == 0 else 21, 0,
                     (biggest + biggest // 255 + 16 + 15) & ~15], name
        want_blocks += [[t, o, n, fixed + n] for (o, n) in wm.block_table(len(d), bs)]
        assert gh + len(written[t][0]) + gt <= g[1], name            # the reference-written container fits its bound
    assert got_blocks == want_blocks
    assert {g[2] for g in got_items} >= {0, 1, 6, 7} and any(g[0] == 0 for g in got_items) and max(g[0] for g in got_items) >= 5


def test_rules_edges(exe, tmp_path):
    """block sizes at the limits, the largest item, every undefined flag, block checksums with kind 1; nibbles 0 .. 15"""
    ok = [(64, 0, 0, 0, 2 ** 31 - 1), (32 << 20, 3, 0xFFFFFFFF, 0xFFFFFFFF, 2 ** 31 - 1), (32 << 20, 0, 0, 0, 1), ((16 << 20) + 1, 0, 0, 0, 0), (1 << 20, 1, 1, 2, 1 << 20)]
    bad = [(63, 0, 0, 0, 5), ((32 << 20) + 1, 0, 0, 0, 5), (64, 0, 0, 0, 2 ** 31), (64, 4, 0, 0, 5), (64, 0x80, 0, 0, 5), (0, 0, 0, 0, 5)]
    rows = [it for it in ok if it[4] // it[0] < 1000] + bad     # (the program prints a line per block)
    got, _ = run_rules(exe, tmp_path, 0, rows)
    for it, g in zip(rows, got):
        if it in bad:
            assert g[6] == 1 and g[0] == 0, it
        else:
            bs, fl, gh, gt, n = it
            assert g[6] == 0 and g[0] == wm.item_blocks(n, bs) and g[1] == wm.item_bound(0, n, bs, fl & 1, gh, gt) and g[2] == wm.level_nibble(bs), it
    got, _ = run_rules(exe, tmp_path, 1, [(64, 1, 0, 0, 5), (64, 2, 0, 0, 5)] + [((1 << k) + 1, 0, 0, 0, 0) for k in range(6, 25)])
    assert got[0][6] == 1 and got[1][6] == 0 and got[1][:2] == [1, 5 + 21]
    assert got[1][7] == 32 and all(g[7] == 16 for g in got[2:])            # 5 bytes, and no bytes, in blocks of up to 16 MiB: slots by what the item holds
    assert [g[2] for g in got[2:]] == [max(0, k + 1 - 10) for k in range(6, 25)]
