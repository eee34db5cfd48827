"""What "right" means for streams whose slots overlap their history, on the CPU and without the engine: the plain definition
(dstream_inorder_common.plain_block -- sequence by sequence, literals first, then the match byte by byte forward, each byte read at the
moment it is due) against the reference library's LZ4_decompress_safe_continue.

The reference equals the plain definition on EVERY block of every minimal-ring stream and of every ring in step with the writer's, and
on EVERY hand-built grid case whose match source lies 31 bytes or more ahead of its destination.  Below 31 it does not: its 32-byte
literal steps (fast loop) and 8-byte steps (safe loop) overwrite the source before the match reads it.  That count is printed and
asserted -- it is the count include/lz4hip.h prints -- so that the stated exception of lz4hip_decompress_safe_stream_inorder_batch stays
visible and header and test cannot drift apart."""
import os

import pytest

from dstream_common import FILL, RefStream, rng_for
from conftest import ROOT
from dstream_inorder_common import count_overlaps, grid, grid_expected, overlap_set, plain_stream

SEED_STREAMS, SEED_GRID = 71, 72      # (the seeds the simulator's and the GPU's tests use too)
GRID_COUNTS = (4290, 1017, 3861)      # cases from 31 bytes ahead on (none differs); cases below that differ, of so many: the header's figures


@pytest.fixture(scope="module")
def rs(ref):
    return RefStream(ref)


def test_reference_is_the_plain_definition_on_every_ring_stream(rs):
    """every block of every m-* and s stream: the reference's decoded bytes, read back directly behind the block's call, are the
    plain definition's -- none left out; a good part of the blocks have slots that overlap the history they can reach"""
    streams = overlap_set(rs, rng_for(SEED_STREAMS), 4)
    blocks = overlaps = 0
    by_layout = {}
    for s in streams:
        w = rs.decode(s, [len(s.blocks)])
        assert all(r >= 0 for r in w.out), (s.name, w.out)
        assert [r for r in w.out] == [b.size for b in s.blocks], s.name          # (and what the writer put in)
        mine = plain_stream(s, w.out)
        assert mine == w.data, (s.name, next(k for k in range(len(mine)) if mine[k] != w.data[k]))
        n = count_overlaps(s, w)
        blocks += len(s.blocks); overlaps += n
        key = s.name.split("#")[0].strip()
        a, b = by_layout.get(key, (0, 0))
        by_layout[key] = (a + len(s.blocks), b + n)
    for k, (a, b) in sorted(by_layout.items()):
        print("%-34s %5d blocks, %5d slots overlap reachable history" % (k, a, b))
    print("%d streams, %d blocks, %d overlapping slots: reference == plain definition on all" % (len(streams), blocks, overlaps))
    assert overlaps >= 500 and any(b for k, (a, b) in by_layout.items() if k.startswith("m-"))


def test_reference_leaves_the_plain_definition_below_31_bytes_ahead_only(rs):
    """the grid, all three tails: from 31 bytes ahead on the reference is the plain definition in every case; below, the count of cases
    where it is not is printed -- and is the count the header states"""
    cases = grid(rng_for(SEED_GRID))
    differ = {}
    total_below = total_from = 0
    for c in cases:
        w = rs.decode(c.stream, [2])
        want, rr = grid_expected(c)
        assert w.out == rr, (c.stream.name, w.out, rr)
        b1 = c.stream.blocks[1]
        same = w.data[1] == want[b1.off:b1.off + rr[1]]
        if c.ahead >= 31:
            total_from += 1
            assert same, c.stream.name
        else:
            total_below += 1
            if not same:
                differ[(c.tail, c.ahead)] = differ.get((c.tail, c.ahead), 0) + 1
    n = sum(differ.values())
    print("grid: %d cases with the source 31 bytes or more ahead, the reference is the plain definition in all of them" % total_from)
    print("grid: %d of %d cases with the source 1 .. 30 bytes ahead differ: %s" % (n, total_below, sorted(differ.items())))
    assert n > 0
    assert all(a <= 8 for (t, a) in differ if t in ("short", "cross"))       # (its safe loop alone: 8-byte steps)
    assert (total_from, n, total_below) == GRID_COUNTS
    text = " ".join(open(os.path.join(ROOT, "include", "lz4hip.h")).read().replace("*", " ").split())
    assert "in %d of the %d cases with a source 1 .. 30 bytes ahead and in none of the %d cases from 31 bytes on" % (n, total_below, total_from) in text
    assert FILL == 0xEE
