#!/usr/bin/env python3
"""The boundary streams of tests/margin_common.py through the lane simulator's loop forms, loop by loop: margin_probe.py [--modes=<letters>] [all|families|<loop name> ...]
prints `loop <name> : cases <n> bad <b> (out of bounds <x>)`.  With LZ4HIP_SIM_FLAGS=<name>:-DLZ4HIP_DECODE_OUT_MARGIN=<v> (or _IN_MARGIN) it runs a
simulator whose margin is weakened: tests/test_margin_hostsim.py's sensitivity tests, and the audit of profiles/decode_margin_audit.txt
(the largest weakened value each loop's cases still catch)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import margin_common as M
import test_margin_hostsim as T
from oracle import oracle as O



def main():
    args = sys.argv[1:] or ["all"]
    modes = T.SIM_MODES
    if args[0].startswith("--modes="):          # only these modes of the case set (the audit: b for the output margin, hi for the input margin)
        modes, args = args[0][8:], args[1:] or ["all"]
    names = list(T.LOOPS) if args == ["all"] else list(T.FAMILIES) if args == ["families"] else args
    cs = M.CaseSet(O.ref(), O)
    sim = T.load_sim()
    for name in names:
        t0 = time.time()
        bad = T.run_loop(sim, cs, T.LOOPS[name], modes=modes, salt=len(name))
        n = sum(c.mode in modes for c in cs.cases)
        by_mode = {m: sum(b[0] == m for b in bad) for m in T.SIM_MODES}
        print("loop %s : cases %d bad %d (out of bounds %d) by mode %s %.1fs" % (name, n, len(bad), sum(b[2] == -1000000 for b in bad), by_mode, time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
