"""Shared pieces of the LZ4_decompress_safe_partial tests (test_partial_hostsim.py, test_partial_abi.py, test_gpu_partial.py): the
reference library's own LZ4_decompress_safe_partial through ctypes, the case matrix, and the one place where liblz4's bytes are not
defined (a cut match of offset 0)."""
import ctypes as C
import random

_u8p = C.POINTER(C.c_uint8)

FIXED_TARGETS = (0, 1, 4, 5, 11, 12, 13, 17, 63, 64, 65, 605, 606, 607)


def ref_partial(ref):
    """(stream, target, cap) -> (ret, dst[:max(ret, 0)]): the reference's LZ4_decompress_safe_partial (never with a negative size)"""
    f = C.CDLL(ref.path).LZ4_decompress_safe_partial
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, _u8p, C.c_int, C.c_int, C.c_int]

    def run(s, t, c, prefill=0xA5):
        assert len(s) >= 0 and t >= 0 and c >= 0
        buf = C.create_string_buffer(bytes(s) + b"\0" * 64, len(s) + 64)   # (slack behind the stream, as the oracle gives liblz4)
        out = (C.c_uint8 * (c + 64))()
        C.memset(out, prefill, c + 64)
        r = f(buf, C.cast(out, _u8p), len(s), t, c)
        return r, bytes(out[:max(r, 0)])
    return run


def undefined_bytes(s, ret, room):
    """positions in [0, ret) that liblz4 leaves as its buffer held them: matches of offset 0 (no compressor emits one) that end
    within 12 bytes of `room` = min(target, cap) -- liblz4's partial branch copies them onto themselves, this engine zero-fills
    them.  Walks the sequences of `s` while they produce output below ret."""
    bad = set()
    i = op = 0
    n = len(s)
    while i < n and op < ret:
        tok = s[i]; i += 1
        lit = tok >> 4
        if lit == 15:
            while i < n:
                x = s[i]; i += 1; lit += x
                if x != 255:
                    break
        op += lit; i += lit
        if i + 2 > n or op >= ret:
            break
        off = s[i] | (s[i + 1] << 8); i += 2
        ml = tok & 15
        if ml == 15:
            while i < n:
                x = s[i]; i += 1; ml += x
                if x != 255:
                    break
        ml += 4
        if off == 0 and op + ml > room - 12:
            bad.update(range(op, min(op + ml, ret)))
        op += ml
    return bad


def same_bytes(got, want, s, ret, room):
    """got == want on every defined position"""
    if got == want:
        return True
    if len(got) != len(want):
        return False
    bad = undefined_bytes(s, ret, room)
    return all(a == b for k, (a, b) in enumerate(zip(got, want)) if k not in bad)


def targets_for(d, rng, n_random=2):
    """the issue's target list for a block of d decoded bytes, plus random ones"""
    ts = set(FIXED_TARGETS) | {max(d - 1, 0), d, d + 1, 2 * d}
    for _ in range(n_random):
        ts.add(rng.randrange(0, d + 2))
    return sorted(ts)


def caps_for(t, rng):
    """capacities below, equal to and above target t"""
    cs = {t, t + rng.randrange(1, 200)}
    if t > 0:
        cs.add(rng.randrange(0, t))
    return sorted(cs)


def overlap_stream(rng, off):
    """a valid block whose first match overlaps its own output: `off` literals (off = 1 .. 15), a long match at distance `off`, then
    five last literals"""
    lit = rng.randbytes(off)
    ml = rng.randrange(20, 700)
    tok_ml = min(ml - 4, 15)
    s = bytearray([(min(off, 15) << 4) | tok_ml]) + (b"\0" if off == 15 else b"") + lit + bytes([off, 0])
    if ml - 4 >= 15:
        v = ml - 4 - 15
        while v >= 255:
            s.append(255); v -= 255
        s.append(v)
    s += bytes([0x50]) + rng.randbytes(5)
    return bytes(s), off + ml + 5


def long_literal_stream():
    """token 0xF0, 8 500 000 bytes of 0xFF, 0x10, then 104 letters: liblz4's 32-bit length sum is past 2^31; the partial decoder cuts
    the run to the input (104 bytes), the full decoder fails"""
    letters = bytes((ord("a") + k % 26) for k in range(104))
    return b"\xf0" + b"\xff" * 8500000 + b"\x10" + letters, letters


def damaged(s, rng, flips=1):
    b = bytearray(s)
    for _ in range(flips):
        if b:
            b[rng.randrange(len(b))] = rng.randrange(256)
    return bytes(b)


def rng_for(seed):
    return random.Random(seed)
