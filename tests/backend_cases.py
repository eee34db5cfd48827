"""The case tables of the backend layer (tests/backend/probes.h): for every family a Launch -- case records, input slots, the
initial output image with its 0xA5 guards, the common image -- and the plain definition of what the probes must leave there
(numpy / Python, a third leg beside the two backends).  tests/test_backend_hostsim.py runs them through the lane simulator's
backends, tests/test_gpu_backend.py through both and compares the images.  A plain module: no test lives here.

Slot layouts are hostsim_backend.cpp's.  An `expect_*` function returns (image, mask): the bytes of `image` where `mask` is set
are what the definition says; the others (what a wild copy may touch past its length, unspecified lanes) are compared between
the two backends only."""
import ctypes as C
import random

import numpy as np

REC, GUARD, FILL = 64, 64, 0xC3
U32 = np.uint32
M32 = 0xFFFFFFFF

# probes.h
(W_BALLOT, W_SHFL, W_SHFL_E, W_BCAST, W_SETLANE, W_ARITH, W_ARITH2) = range(7)
(W_LD, W_LDU, W_ST8, W_ST32, W_ST16, W_LANES, W_COPY) = range(10, 17)
(W_LDS_FILL, W_LDS_WR, W_LDS_MAX) = range(20, 23)
(G_MATCH, G_MATCH_WIDE, G_LITS, G_LITS_WIDE, G_SEQ, G_STAGE) = range(6)
(S_LITS, S_MATCH, S_FLUSH_LINES, S_FLUSH_ALL) = range(4)
B_WALK, B_LANEOPS, B_LANE_RW, B_GATHER, B_WIN, B_PUT, B_RUN = 0, 1, 2, 3, 4, 5, 6
K_WAVE_VEC, K_WAVE_DATA, K_WAVE_HDR, K_WAVE_OB = 1024, 1152, 1024, 1088
K_STAGE, K_FAR, LDS_BYTES = 576, 8192 + 128, 32768      # (checked against the libraries: assert_constants)
WAVE_CFG = [(8192, 1024), (16384, 2048), (32768, 2048), (65536, 2048)]   # decode_wave.hip's launch table
GLS = [4, 8, 16, 32, 64]


class Launch:
    """One launch of one family: rec (n x 64 words), inp (n x in_stride bytes), out (n x out_stride bytes, the image before the
    run), common (bytes), names (what each case is, for messages)"""

    def __init__(self, family, param, rec, inp, out, common=b"", names=None):
        self.family, self.param = family, param
        self.rec = np.ascontiguousarray(rec, dtype=U32)
        self.inp = np.ascontiguousarray(inp, dtype=np.uint8)
        self.out = np.ascontiguousarray(out, dtype=np.uint8)
        self.common = np.frombuffer(bytes(common) or b"\0\0\0\0", dtype=np.uint8)
        self.n = self.rec.shape[0]
        self.names = names or [""] * self.n
        assert self.rec.shape == (self.n, REC) and self.inp.shape[0] == self.n and self.out.shape[0] == self.n

    def describe(self, i):
        return "family %s%s case %d (%s) record %s" % (self.family, "" if self.param is None else "[%s]" % (self.param,), i, self.names[i],
                                                       [int(x) for x in self.rec[i][:16]])

    def chunks(self, limit=60 << 20):
        """the launch cut into launches of at most `limit` bytes of images (the big rings)"""
        per = max(1, limit // (self.inp.shape[1] + self.out.shape[1]))
        for s in range(0, self.n, per):
            yield s, Launch(self.family, self.param, self.rec[s:s + per], self.inp[s:s + per], self.out[s:s + per], self.common, self.names[s:s + per])


def _ptr(a, t=C.c_uint8):
    return a.ctypes.data_as(C.POINTER(t))


def _call(fn, L, out, extra):
    args = []
    if L.family in ("B",):
        args.append(C.c_int(L.param))
    if L.family in ("C",):
        args.append(C.c_int(WAVE_CFG.index(L.param)))
    args += [_ptr(L.rec, C.c_uint32), C.c_int(L.n)]
    if L.family == "C":
        args += [_ptr(L.common), C.c_size_t(L.common.size)]
    args += [_ptr(L.inp), C.c_size_t(L.inp.shape[1]), _ptr(out), C.c_size_t(out.shape[1])] + extra
    fn.restype = C.c_int
    return fn(*args)


_ENTRY = {"A": "wave", "B": "group", "C": "bwave"}


def assert_constants(lib, entry):
    """the layout constants and backend facts this module restates (the flush model's kStage among them) are the library's own:
    hb_constants / devprobe_constants report probes.h's and the backends' values"""
    got = (C.c_uint32 * 8)()
    getattr(lib, entry)(got)
    want = [REC, GUARD, K_WAVE_VEC, K_WAVE_DATA, K_WAVE_OB, K_FAR, K_STAGE, LDS_BYTES]
    assert list(got) == want, (entry, list(got), want)


def run_host(lib, L):
    """-> (output image, oob flag per case) of the lane simulator's backends"""
    out, oob = L.out.copy(), np.zeros(L.n, dtype=np.uint8)
    assert _call(getattr(lib, "hb_" + _ENTRY[L.family]), L, out, [_ptr(oob)]) == 0
    return out, oob


def run_dev(lib, L):
    """-> (HIP error code, output image) of the device backends; the launch goes in chunks of at most 60 MB of images"""
    out = L.out.copy()
    for s, part in L.chunks():
        o = part.out.copy()
        code = _call(getattr(lib, "devprobe_" + _ENTRY[L.family]), part, o, [])
        if code:
            return code, out
        out[s:s + part.n] = o
    return 0, out


def assert_no_oob(L, oob):
    bad = np.flatnonzero(oob)
    assert bad.size == 0, "%d cases leave their slot or LDS layout (oob), the first: %s" % (bad.size, L.describe(int(bad[0])))


def assert_same(L, got, want, mask=None, what="the two backends differ"):
    """byte for byte (where mask is set); the message names the family, the case record and the first differing byte"""
    d = got != want
    if mask is not None:
        d &= mask
    if d.any():
        i = int(np.flatnonzero(d.any(axis=1))[0])
        k = int(np.flatnonzero(d[i])[0])
        raise AssertionError("%s: %s, first at byte %d of the slot (word %d, lane %d): %#x, expected %#x; %d bytes differ in this case, %d cases differ"
                             % (what, L.describe(i), k, k // 4, (k // 4) % 64, int(got[i, k]), int(want[i, k]), int(d[i].sum()), int(d.any(axis=1).sum())))


def unspecified(L):
    """mask of the bytes that are compared between the backends: everything but what is documented as unspecified"""
    m = np.ones(L.out.shape, dtype=bool)
    if L.family == "A":
        op = L.rec[:, 0]
        m[op == W_SHFL, GUARD + 768 + 63 * 4:GUARD + 768 + 64 * 4] = False          # lane 63 of shfl_down1
        m[op == W_LDS_MAX, GUARD:GUARD + 512] = False                                   # lds_max's old values: the hardware's order
    return m


# ---------------------------------------------------------------------------------------------------------------- family A
def _wave_out(n, payload):
    out = np.full((n, GUARD + payload + GUARD), FILL, dtype=np.uint8)
    out[:, :GUARD] = 0xA5
    out[:, -GUARD:] = 0xA5
    return out


def _words(img, off, count=64):
    """view of `count` words at byte offset `off` of every slot's payload"""
    return img[:, GUARD + off:GUARD + off + 4 * count].view(U32)


def wave_value_cases(seed=1, nrandom=2000):
    rng = np.random.default_rng(seed)
    base = [rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(U32) for _ in range(nrandom)]
    base += [np.zeros(64, U32), np.full(64, M32, U32), np.arange(64, dtype=U32)]
    for l in range(64):
        v = np.zeros(64, U32)
        v[l] = U32(rng.integers(1, 1 << 32))
        base.append(v)
    ops = [W_BALLOT, W_SHFL, W_SHFL_E, W_BCAST, W_SETLANE, W_ARITH, W_ARITH2]
    n = len(base) * len(ops)
    rec = np.zeros((n, REC), U32)
    vec = rng.integers(0, 1 << 32, (n, 4, 64), dtype=np.uint64).astype(U32)
    names = []
    for i in range(n):
        op, a = ops[i % len(ops)], base[i // len(ops)]
        k = i // len(ops)
        vec[i, 0] = a
        rec[i, 0] = op
        names.append("op %d vector %d" % (op, k))
        if k >= nrandom:                       # the special vectors: d of the same kind (64-bit operands), masks of the same kind
            vec[i, 3] = a
        if op == W_BALLOT:
            m = [int(rng.integers(0, 1 << 64, dtype=np.uint64)), 0, (1 << 64) - 1, 1 << (k % 64)][k % 4 if k % 5 == 0 else 0]
            rec[i, 2], rec[i, 3] = m & M32, m >> 32
        if op in (W_SHFL, W_SHFL_E) and k % 2:
            vec[i, 1] &= 63
        if op in (W_BCAST, W_SETLANE):
            rec[i, 2], rec[i, 3] = k % 64, int(rng.integers(0, 1 << 32))
        if op == W_ARITH:
            vec[i, 2] = rng.integers(0, 64, 64)                       # shr: shift amounts 0 .. 63; alignbyte: sh 0 .. 3
            vec[i, 0, 4:10] = [0, 254, 255, 256, M32, 255 * 65536]
        if op == W_ARITH2:                                            # clz64 / ctz64v: 0, 1, 1 << 63, all ones
            vec[i, 0, 0:4] = [0, 1, 0, M32]
            vec[i, 3, 0:4] = [0, 0, 1 << 31, M32]
    inp = vec.reshape(n, 256).view(np.uint8)
    return Launch("A", None, rec, inp, _wave_out(n, K_WAVE_OB), names=names)


def expect_wave_value(L):
    img = L.out.copy()
    v = L.inp.view(U32).reshape(L.n, 4, 64).astype(np.uint64)
    A, Bv, Cv, D = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
    X = A | (D << np.uint64(32))
    lane = np.arange(64, dtype=np.uint64)
    O = [_words(img, 256 * k) for k in range(4)]
    H0, H1 = _words(img, K_WAVE_HDR, 4), _words(img, K_WAVE_HDR + 16, 4)
    op = L.rec[:, 0]
    s2, s3 = L.rec[:, 2].astype(np.uint64), L.rec[:, 3].astype(np.uint64)
    rows = np.arange(L.n)[:, None]
    pick = lambda V, idx: V[rows, (idx & np.uint64(63)).astype(np.int64)]

    def put(dst, sel, val):
        dst[sel] = (val[sel] & np.uint64(M32)).astype(U32)

    s = op == W_BALLOT
    m = ((A & np.uint64(1)) << lane).sum(axis=1, dtype=np.uint64)
    H0[s, 0], H0[s, 1], H0[s, 2], H0[s, 3] = (m[s] & np.uint64(M32)).astype(U32), (m[s] >> np.uint64(32)).astype(U32), 0, 0
    m2 = (s2 | (s3 << np.uint64(32)))[:, None]
    bit = (m2 >> lane) & np.uint64(1)
    put(O[0], s, np.where(bit == 1, A, Bv))
    put(O[1], s, np.cumsum(bit, axis=1, dtype=np.uint64) - bit)
    lt = (np.uint64(1) << lane) - np.uint64(1)
    put(O[2], s, np.broadcast_to(lt, A.shape))
    put(O[3], s, np.broadcast_to(lt >> np.uint64(32), A.shape))
    s = op == W_SHFL
    put(O[0], s, np.cumsum(A, axis=1, dtype=np.uint64) - A)            # the serial prefix sum
    put(O[1], s, pick(A, Bv))
    put(O[2], s, np.concatenate([A[:, :1], A[:, :-1]], axis=1))
    put(O[3], s, np.concatenate([A[:, 1:], A[:, -1:]], axis=1))      # (lane 63: masked)
    s = op == W_SHFL_E
    put(O[0], s, pick(A, Bv)); put(O[1], s, pick(D, Bv)); put(O[2], s, pick(A, Bv))
    s = op == W_BCAST
    al, dl = pick(A, s2[:, None])[:, 0], pick(D, s2[:, None])[:, 0]
    for k, val in enumerate([al, al, dl, al]):
        H0[s, k] = val[s].astype(U32)
    for k, val in enumerate([al, dl, al * np.uint64(0), al * np.uint64(0)]):
        H1[s, k] = val[s].astype(U32)
    s = op == W_SETLANE
    setl = np.where(lane[None, :] == s2[:, None], s3[:, None], A)
    put(O[0], s, setl); put(O[1], s, setl)
    s = op == W_ARITH
    put(O[0], s, ((A << np.uint64(32)) | Bv) >> (np.uint64(8) * (Cv & np.uint64(3))))
    put(O[1], s, A // np.uint64(255))
    put(O[2], s, A >> (Cv & np.uint64(31)))
    put(O[3], s, np.minimum(A, Bv))
    s = op == W_ARITH2
    put(O[0], s, np.maximum(A, Bv))
    clz = np.full(A.shape, 64, np.uint64)
    ctz = np.full(A.shape, 64, np.uint64)
    for i in np.flatnonzero(s):
        for l in range(64):
            x = int(X[i, l])
            if x:
                clz[i, l], ctz[i, l] = 64 - x.bit_length(), (x & -x).bit_length() - 1
    put(O[1], s, clz); put(O[2], s, ctz)
    put(O[3], s, np.where((Cv & np.uint64(1)) == 1, A, Bv))
    return img, unspecified(L)


def wave_mem_cases(seed=2):
    rng = np.random.default_rng(seed)
    recs, vecs, names = [], [], []

    def add(op, name, b=None, c=None, d=None, **r):
        rec = np.zeros(REC, U32)
        rec[0] = op
        for k, val in r.items():
            rec[int(k[1:])] = val
        v = rng.integers(0, 1 << 32, (4, 64), dtype=np.uint64).astype(U32)
        for k, val in ((1, b), (2, c), (3, d)):
            if val is not None:
                v[k] = val
        recs.append(rec); vecs.append(v); names.append(name)

    for t in range(200):     # masked and unmasked loads: random indices at every alignment mod 8 (lane l of case t: l + t mod 8)
        idx = (rng.integers(0, (K_WAVE_DATA - 16) // 8, 64) * 8 + (np.arange(64) + t) % 8).astype(U32)
        add(W_LD, "ld8/32/64 %d" % t, b=idx)
        add(W_LDU, "ldu8/32/64 sld32 %d" % t, b=idx, d=idx[::-1].copy(), r2=int(rng.integers(0, K_WAVE_DATA - 4)))
    for t in range(100):
        add(W_ST8, "st8 %d" % t, b=rng.permutation(K_WAVE_DATA)[:64].astype(U32))
        cells = rng.permutation(K_WAVE_DATA // 12)[:64]
        add(W_ST32, "st32 %d" % t, b=(cells * 12 + (np.arange(64) + t) % 8).astype(U32))
        add(W_ST16, "st16 %d" % t, b=rng.permutation(K_WAVE_DATA // 2)[:64].astype(U32))
    for t in range(50):
        add(W_LANES, "st_lanes/ld_lanes st_hdr/ld_hdr %d" % t, r2=int(rng.integers(0, 253)))
    al = [0, 1, 3, 15]
    # copy: every length (a body of two rounds of 1024 bytes, every tail).  All 16 (destination, source) alignment pairs for the lengths
    # below 80 and above 1020 -- every tail behind zero to four chunks, and the second round -- ; in between every length sees every
    # source and every destination alignment once, the pairs rotating with the length (copy moves unaligned 16-byte chunks: no path
    # of it depends on the pair)
    for n in range(1101):
        pairs = [(dal, sal) for dal in al for sal in al] if n < 80 or n > 1020 else [(al[(k + n) % 4], al[k]) for k in range(4)]
        for dal, sal in pairs:
            add(W_COPY, "copy len %d to %d from %d" % (n, dal, sal), r2=dal, r3=sal, r4=n)
    n = len(recs)
    inp = np.zeros((n, K_WAVE_VEC + K_WAVE_DATA), np.uint8)
    inp[:, :K_WAVE_VEC] = np.array(vecs).reshape(n, 256).view(np.uint8)
    inp[:, K_WAVE_VEC:] = rng.integers(0, 256, (n, K_WAVE_DATA), dtype=np.uint8)
    return Launch("A", None, np.array(recs), inp, _wave_out(n, K_WAVE_OB + K_WAVE_DATA), names=names)


def expect_wave_mem(L):
    img = L.out.copy()
    v = L.inp[:, :K_WAVE_VEC].view(U32).reshape(L.n, 4, 64)
    data = L.inp[:, K_WAVE_VEC:]
    O = [_words(img, 256 * k) for k in range(4)]
    H0 = _words(img, K_WAVE_HDR, 4)
    ob = img[:, GUARD + K_WAVE_OB:GUARD + K_WAVE_OB + K_WAVE_DATA]
    le = lambda by: int.from_bytes(bytes(by), "little")
    for i in range(L.n):
        op, r = int(L.rec[i, 0]), L.rec[i]
        a, b, c, d = (v[i, k] for k in range(4))
        on = (c & 1) == 1
        if op in (W_LD, W_LDU):
            m = on if op == W_LD else np.ones(64, bool)
            for l in range(64):
                p = int(b[l])
                O[0][i, l] = data[i, p] if m[l] else 0
                O[1][i, l] = le(data[i, p:p + 4]) if m[l] else 0
                O[2][i, l] = le(data[i, p:p + 4]) if m[l] else 0
                O[3][i, l] = le(data[i, p + 4:p + 8]) if m[l] else 0
                if op == W_LDU:
                    q = int(d[l])
                    O[3][i, l] ^= le(data[i, q:q + 4]) ^ le(data[i, q + 4:q + 8])
            if op == W_LDU:
                H0[i] = [le(data[i, int(r[2]):int(r[2]) + 4]), 0, 0, 0]
        elif op in (W_ST8, W_ST32, W_ST16):
            w = {W_ST8: 1, W_ST32: 4, W_ST16: 2}[op]
            for l in np.flatnonzero(on):
                p = int(b[l]) * (2 if op == W_ST16 else 1)
                ob[i, p:p + w] = np.frombuffer(int(a[l]).to_bytes(4, "little")[:w], np.uint8)
        elif op == W_LANES:
            h = L.inp[i].view(U32)[int(r[2]):int(r[2]) + 4]
            H0[i] = h[::-1]
            O[0][i] = b
        elif op == W_COPY:
            ob[i, int(r[2]):int(r[2]) + int(r[4])] = data[i, int(r[3]):int(r[3]) + int(r[4])]      # memcpy
    return img, unspecified(L)


def wave_lds_cases(seed=3):
    rng = np.random.default_rng(seed)
    recs, vecs, names = [], [], []

    def add(op, u16, name, b=None, c=None, d=None, **r):
        rec = np.zeros(REC, U32)
        rec[0], rec[1], rec[5] = op, u16, LDS_BYTES // (4 if u16 else 8)
        for k, val in r.items():
            rec[int(k[1:])] = val
        v = rng.integers(0, 1 << 32, (4, 64), dtype=np.uint64).astype(U32)
        for k, val in ((1, b), (2, c), (3, d)):
            if val is not None:
                v[k] = val
        recs.append(rec); vecs.append(v); names.append(name + (" u32" if u16 else " u64"))

    for u16 in (1, 0):
        full = LDS_BYTES // (4 if u16 else 8)
        for count in (0, 1, 63, 64, 65, full):
            add(W_LDS_FILL, u16, "lds_fill %d" % count, r2=count, r3=int(rng.integers(1, 1 << 32)), r4=int(rng.integers(1, 1 << 32)))
        for t in range(60):
            slots = rng.permutation(full)[:64].astype(U32)
            rd = np.where(rng.integers(0, 2, 64) == 1, rng.permutation(slots), rng.integers(0, full, 64)).astype(U32)
            # (with 64-bit entries d is the values' upper half as well as the read slots)
            add(W_LDS_WR, u16, "lds_wr/rd/rdu %d" % t, b=slots, d=rd, r3=int(rng.integers(0, 1 << 32)), r4=int(rng.integers(0, 1 << 32)))
        for t in range(100):
            kind = t % 5
            if kind == 0: slots = rng.permutation(full)[:64]                               # no collision
            elif kind == 1: slots = np.repeat(rng.permutation(full)[:32], 2)               # collisions of 2
            elif kind == 2: slots = np.resize(np.repeat(rng.permutation(full)[:22], 3), 64)   # of 3 (and one of 1)
            elif kind == 3: slots = np.full(64, rng.integers(0, full))                     # all 64 lanes on one slot
            else: slots = rng.integers(0, 8, 64) + rng.integers(0, full - 8)                # random, dense
            # the initial value in the middle of the values' range: some lanes raise the slot, some do not
            # every other case of a kind with all 64 lanes active (the collisions are then exactly the kind's: 2, 3, all 64 lanes on one
            # slot), the others under a random mask
            allon = (t // 5) % 2 == 0
            add(W_LDS_MAX, u16, "lds_max %d kind %d%s" % (t, kind, "" if allon else " masked"), b=rng.permutation(slots).astype(U32),
                c=np.full(64, M32, U32) if allon else None, r3=1 << 31, r4=1 << 31)
    n = len(recs)
    inp = np.array(vecs).reshape(n, 256).view(np.uint8)
    return Launch("A", None, np.array(recs), inp, _wave_out(n, K_WAVE_OB + LDS_BYTES), names=names)


def lds_max_collisions(L):
    """-> {entry width: the set of numbers of ACTIVE lanes that meet on one slot, over all lds_max cases}"""
    seen = {True: set(), False: set()}
    for i in np.flatnonzero(L.rec[:, 0] == W_LDS_MAX):
        u16, v, _, _ = _lds_case(L, i)
        on = (v[2] & np.uint64(1)) == 1
        seen[u16] |= {int(x) for x in np.unique(v[1][on], return_counts=True)[1]}
    return seen


def _lds_case(L, i):
    r = L.rec[i]
    u16 = bool(r[1])
    v = L.inp[i].view(U32).reshape(4, 64).astype(np.uint64)
    val = v[0] if u16 else v[0] | (v[3] << np.uint64(32))
    sval = int(r[3]) if u16 else int(r[3]) | (int(r[4]) << 32)
    return u16, v, val, sval


def expect_wave_lds(L):
    img = L.out.copy()
    mask = unspecified(L)
    for i in range(L.n):
        op, r = int(L.rec[i, 0]), L.rec[i]
        u16, v, val, sval = _lds_case(L, i)
        full = LDS_BYTES // (4 if u16 else 8)
        tab = np.zeros(full, np.uint64)
        on = (v[2] & np.uint64(1)) == 1
        b = v[1].astype(np.int64)

        def wr(word, x):    # an entry vector: one word per lane, or two
            _words(img, 4 * word)[i] = (x & np.uint64(M32)).astype(U32)
            if not u16:
                _words(img, 4 * word + 256)[i] = (x >> np.uint64(32)).astype(U32)

        if op == W_LDS_FILL:
            tab[:int(r[2])] = sval
        elif op == W_LDS_WR:
            tab[:] = sval
            tab[b[on]] = val[on]
            d = v[3].astype(np.int64)
            wr(0, np.where((v[2] & np.uint64(2)) != 0, tab[d], np.uint64(0)))
            wr(128, tab[d])
        else:
            tab[:] = sval
            np.maximum.at(tab, b[on], val[on])
        dump = img[i, GUARD + K_WAVE_OB:GUARD + K_WAVE_OB + LDS_BYTES].view(U32)
        if u16:
            dump[:] = tab.astype(U32)
        else:   # per 64 entries: the lower words, then the upper words
            t2 = tab.reshape(-1, 64)
            dump.reshape(-1, 2, 64)[:, 0] = (t2 & np.uint64(M32)).astype(U32)
            dump.reshape(-1, 2, 64)[:, 1] = (t2 >> np.uint64(32)).astype(U32)
    return img, mask


def check_lds_max_old(L, out, who):
    """lds_max's returned old values against the definition of an atomic max, whatever order the lanes were served in: each is the
    slot's initial value or another colliding lane's value, none exceeds the final value, per slot at least one lane sees the
    initial value"""
    for i in np.flatnonzero(L.rec[:, 0] == W_LDS_MAX):
        u16, v, val, sval = _lds_case(L, i)
        on = (v[2] & np.uint64(1)) == 1
        old = _words(out, 0)[i].astype(np.uint64)
        if not u16:
            old |= _words(out, 256)[i].astype(np.uint64) << np.uint64(32)
        assert (old[~on] == 0).all(), (who, L.describe(i), "an inactive lane returned a value")
        for slot in np.unique(v[1][on]):
            lanes = np.flatnonzero(on & (v[1] == slot))
            final = max(sval, int(val[lanes].max()))
            seen_initial = False
            for l in lanes:
                others = {int(val[k]) for k in lanes if k != l}
                assert int(old[l]) == sval or int(old[l]) in others, (who, L.describe(i), "lane %d: old value %#x is neither the initial value nor a colliding lane's" % (l, int(old[l])))
                assert int(old[l]) <= final, (who, L.describe(i), "lane %d: old value above the final value" % l)
                seen_initial |= int(old[l]) == sval
            assert seen_initial, (who, L.describe(i), "slot %d: no lane saw the initial value" % int(slot))


# ---------------------------------------------------------------------------------------------------------------- family B
def _lb(gl):
    return max(4, 64 // gl)


def _group_launch(gl, recs, names, in_stride, out_stride, rng):
    n = len(recs)
    out = np.full((n, out_stride), 0xA5, dtype=np.uint8)
    rec = np.array(recs, dtype=U32)
    cap = out_stride - 384
    for i in range(n):   # the destination: random bytes (history and what lies behind the copy alike)
        o = 128 + int(rec[i, 7])
        out[i, o:o + cap] = rng.integers(0, 256, cap, dtype=np.uint8)
    out[:, out_stride - 128:out_stride - 124] = FILL
    inp = rng.integers(0, 256, (n, in_stride), dtype=np.uint8)
    return Launch("B", gl, rec, inp, out, names=names)


def _uniq(xs):
    return sorted({int(x) for x in xs if x >= 0})


HIST = 512     # the copies' output position: room for an offset of 300 and a far sequence source in front of it


def group_copy_cases(gl, seed=4):
    rng = np.random.default_rng(seed + gl)
    step = _lb(gl) * gl
    offsets = _uniq([0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, gl - 1, gl, gl + 1, 4 * gl - 1, 4 * gl, 4 * gl + 1, step - 1, step, step + 1, 300])
    lens = _uniq([0, 1, 2, 3, 4, 5, gl - 1, gl, gl + 1, 4 * gl - 1, 4 * gl, 4 * gl + 1, step - 1, step, step + 1, 2 * step + 3, 3 * step + 5])
    recs, names = [], []

    def add(name, op, al, *p):
        r = np.zeros(REC, U32)
        r[0], r[2] = op, HIST
        r[3:3 + len(p)] = p
        r[7] = (al - HIST) % 128          # the address of dst + op is `al` mod 128
        recs.append(r); names.append(name)

    for al in (0, 1, 3, 127):
        for off in offsets:
            for ln in lens:
                add("copy_match offset %d len %d" % (off, ln), G_MATCH, al, off, ln, 0)
                add("copy_match wild offset %d len %d" % (off, ln), G_MATCH, al, off, ln, 1)
                add("copy_match_wide offset %d len %d" % (off, ln), G_MATCH_WIDE, al, off, ln)
        for sal in (0, 1, 3):
            for ln in lens:
                add("copy_lits len %d" % ln, G_LITS, al, sal, ln, 0)
                add("copy_lits wild len %d" % ln, G_LITS, al, sal, ln, 1)
                add("copy_lits_wide len %d" % ln, G_LITS_WIDE, al, sal, ln)
    lb = _lb(gl)
    sizes = _uniq([0, 1, lb - 1, lb, lb + 1, step - lb, step - 1, step])
    for k, (lit, ln) in enumerate((a, b) for a in sizes for b in sizes):
        # the distance: at least a step, and what the interior loop asks of a "simple" sequence (lz4_decode_core.h: the source ends
        # a slack in front of the sequence's own output)
        d0 = max(step, lit + ln + lb)
        for dist in (d0, d0 + 1, max(d0, HIST - (k % 5))):
            add("seq_load/seq_store lit %d len %d distance %d" % (lit, ln, dist), G_SEQ, (0, 1, 3, 127)[k % 4], k % 4, lit, dist, ln)
    return _group_launch(gl, recs, names, 2048, 2048, rng)


def expect_group_copy(L):
    img = L.out.copy()
    mask = np.ones(img.shape, bool)
    gl = L.param
    for i in range(L.n):
        r = [int(x) for x in L.rec[i][:8]]
        op, o = r[0], 128 + r[7]
        d = img[i, o:]                                # (a view: dst)
        touched = mask[i, o:]
        src = L.inp[i]
        if op in (G_MATCH, G_MATCH_WIDE):
            pos, off, ln = r[2], r[3], r[4]
            for k in range(ln):                       # byte-forward LZ4 match copy
                d[pos + k] = d[pos + k - off] if off else 0
            wild = op == G_MATCH_WIDE or r[5]
            touched[pos + ln:pos + ln + (max(_lb(gl), 4) if wild else 0)] = False
        elif op in (G_LITS, G_LITS_WIDE):
            pos, sp, ln = r[2], r[3], r[4]
            d[pos:pos + ln] = src[sp:sp + ln]
            wild = op == G_LITS_WIDE or r[5]
            touched[pos + ln:pos + ln + (max(_lb(gl), 4) if wild else 0)] = False
        else:
            pos, sp, lit, dist, ln = r[2], r[3], r[4], r[5], r[6]
            d[pos:pos + lit] = src[sp:sp + lit]
            d[pos + lit:pos + lit + ln] = d[pos + lit - dist:pos + lit - dist + ln].copy()
            # (a step's chunks reach up to LB - 1 bytes past each part: the match part's first bytes are then the match's own)
            touched[pos + lit + ln:pos + lit + ln + _lb(gl)] = False
            if ln == 0:
                touched[pos + lit:pos + lit + _lb(gl)] = False
    return img, mask


def _stage_script(gl, dst_al, ops, name, hand=False):
    """ops: ("lits", len) / ("match", offset, len) / ("lines",) / ("all",) / ("all_at", bytes back from the current position).  Positions
    are filled in here, and so is st_match's precondition: its source lies in flushed memory, so a flush of everything is put in front
    of it where it does not (for that, fl is followed by the backends' flush rule; expect_group_stage follows it again from the finished
    record, on its own).  A script is at most 12 operations: a random one is cut there, a hand-built one must fit.  -> (record, name)"""
    lb, step = _lb(gl), _lb(gl) * gl
    r = np.zeros(REC, U32)
    pos0 = 640
    r[0], r[2], r[7] = G_STAGE, pos0, (dst_al - pos0) % 128
    script, pos, sp = [], pos0, 0
    fl = pos0
    base = 128 + int(r[7])     # dst's offset in the (256-byte aligned) slot: its address mod 128

    def lines(p):
        nonlocal fl
        t = p - ((base + p) & 127)
        if t > fl:
            fl = t

    def room(p, ln):
        for b in range(0, ln, step):
            if p + b - fl + step + lb > K_STAGE:
                lines(p + b)

    for o in ops:
        if o[0] == "lits":
            script.append((S_LITS, pos, sp, o[1])); room(pos, o[1]); pos += o[1]; sp += o[1]
        elif o[0] == "match":
            off, ln = max(o[1], step, o[2] + lb), o[2]
            if pos - off < 0:
                continue
            if pos - off + ln + lb > fl:
                script.append((S_FLUSH_ALL, pos, 0, 0)); fl = max(fl, pos)
            script.append((S_MATCH, pos, off, ln)); room(pos, ln); pos += ln
        elif o[0] == "lines":
            script.append((S_FLUSH_LINES, pos, 0, 0)); lines(pos)
        elif o[0] == "all":
            script.append((S_FLUSH_ALL, pos, 0, 0)); fl = max(fl, pos)
        else:
            script.append((S_FLUSH_ALL, pos - o[1], 0, 0)); fl = max(fl, pos - o[1])
    assert not hand or len(script) <= 12, (name, len(script))
    script = script[:12]
    r[1] = len(script)
    for k, s in enumerate(script):
        r[8 + 4 * k:12 + 4 * k] = s
    return r, name


def group_stage_cases(gl, seed=5, nrandom=200):
    rng = random.Random(seed * 100 + gl)
    lb, step = _lb(gl), _lb(gl) * gl
    recs, names = [], []
    als = (0, 1, 77, 127)
    near = K_STAGE - step - lb
    hand = []
    for d in (-1, 0, 1):    # the buffer filled to within one step of kStage: the flush inside st_lits / st_match fires (or just does not)
        hand.append([("lits", near + d), ("lits", step), ("all",)])
        hand.append([("lits", near + d), ("match", step, step), ("all",)])
        hand.append([("lits", near + d), ("lits", 1), ("lits", 2 * step + 3)])
    for ln in (0, 1, 100, 127, 128, 129, 255, 256, 257):   # a flush whose target is exactly fl, one line above it, two
        hand.append([("lits", ln), ("lines",), ("lits", 5), ("lines",)])
    for ln in (600, 700, 1000):                            # st_flush_all at a position that st_lits has already flushed past
        hand.append([("lits", 40), ("lits", ln), ("all_at", ln)])
        hand.append([("lits", ln), ("all_at", ln), ("lits", 3), ("all",)])
    for h in hand:
        for al in als:
            r, nm = _stage_script(gl, al, h, "hand-built %s at %d mod 128" % (h, al), hand=True)
            recs.append(r); names.append(nm)
    for t in range(nrandom):
        ops = []
        for _ in range(rng.randrange(1, 12)):
            k = rng.random()
            ln = rng.choice([rng.randrange(0, 20), rng.randrange(0, step + 2), rng.randrange(0, 3 * step)])
            ln = min(ln, 400)
            if k < 0.45: ops.append(("lits", ln))
            elif k < 0.8: ops.append(("match", rng.choice([step, step + 1, rng.randrange(step, 600)]), ln))
            elif k < 0.9: ops.append(("lines",))
            else: ops.append(("all",))
        r, nm = _stage_script(gl, als[t % 4], ops, "random script %d at %d mod 128" % (t, als[t % 4]))
        recs.append(r); names.append(nm)
    return _group_launch(gl, recs, names, 4608, 5632, np.random.default_rng(seed + gl))


def expect_group_stage(L):
    """the logical output of the script (literals from the source, matches byte-forward) in [start, fl); fl itself by the flush rule
    (whole 128-byte lines of the address leave; a flush of everything leaves all).  What lies at and above fl -- up to LB - 1 bytes
    that a flush carries along -- is compared between the backends only"""
    img = L.out.copy()
    mask = np.ones(img.shape, bool)
    gl = L.param
    lb, step = _lb(gl), _lb(gl) * gl
    for i in range(L.n):
        r = L.rec[i]
        base = 128 + int(r[7])
        logical = img[i, base:].copy()
        fl = pos0 = int(r[2])
        src = L.inp[i]

        def lines(p):
            t = p - ((base + p) & 127)
            return max(fl, t)

        for k in range(int(r[1])):
            kind, p, x, y = (int(v) for v in r[8 + 4 * k:12 + 4 * k])
            if kind in (S_LITS, S_MATCH):
                for b in range(0, y, step):
                    if p + b - fl + step + lb > K_STAGE:
                        fl = lines(p + b)
                if kind == S_LITS:
                    logical[p:p + y] = src[x:x + y]
                else:
                    for j in range(y):
                        logical[p + j] = logical[p + j - x]
            elif kind == S_FLUSH_LINES:
                fl = lines(p)
            else:
                fl = max(fl, p)
        img[i, base + pos0:base + fl] = logical[pos0:fl]
        mask[i, base + fl:base + fl + lb] = False
        img[i, L.out.shape[1] - 128:L.out.shape[1] - 124] = np.frombuffer(int(fl).to_bytes(4, "little"), np.uint8)
    return img, mask


# ---------------------------------------------------------------------------------------------------------------- family C
def walk_tables():
    """the 3000 tables of test_wave_walk_asm_text_in_the_interpreter (same generator, same seed), then tables with exactly 60 .. 64 and
    84 starts and the single-start table"""
    rng = random.Random(31337)
    tabs = []
    for trial in range(3000):
        gap = rng.choice([3, 4, 6, 10, 30, 80, 300])
        nxt = [255] * 256
        for p_ in range(256):
            q = p_ + rng.randrange(3, gap + 1)
            nxt[p_] = q if q <= 250 else 255
        if trial % 50 == 0:
            nxt[0] = 255
        if trial % 50 == 1:
            for p_ in range(0, 250, 3): nxt[p_] = p_ + 3 if p_ + 3 <= 250 else 255
        tabs.append(nxt)
    for starts in (60, 61, 62, 63, 64, 84):
        for fillv in (255, 7):     # what the positions off the chain hold: nothing, or a pointer into the chain
            nxt = [fillv if p_ < 248 else 255 for p_ in range(256)]
            for k in range(starts):
                nxt[3 * k] = 3 * k + 3 if k + 1 < starts else 255
            tabs.append(nxt)
    single = [255] * 256
    tabs.append(single)
    return tabs


def walk_definition(nxt):
    want, s = [], 0
    while True:
        want.append(s)
        s = nxt[s]
        if s == 255 or len(want) == 64:
            return want


def _bwave_out(n, stride):
    out = np.full((n, stride), 0xA5, dtype=np.uint8)
    out[:, 256:256 + 1280] = FILL
    return out


def bwave_lane_cases(cfg, seed=6):
    rng = np.random.default_rng(seed)
    tabs = walk_tables()
    recs, vecs, names = [], [], []

    def add(op, name, vec=None, **r):
        rec = np.zeros(REC, U32)
        rec[0] = op
        for k, val in r.items():
            rec[int(k[1:])] = val
        v = rng.integers(0, 1 << 32, (5, 64), dtype=np.uint64).astype(U32)
        for k, val in (vec or {}).items():
            v[k] = val
        recs.append(rec); vecs.append(v); names.append(name)

    for t, nxt in enumerate(tabs):
        add(B_WALK, "vwalk / vwalk_par table %d" % t, {0: np.frombuffer(bytes(nxt), dtype=U32)})
    for t in range(300):
        a = [None, np.zeros(64, U32), np.full(64, M32, U32), np.arange(64, dtype=U32)][t % 4 if t < 16 else 0]
        add(B_LANEOPS, "vexcl_scan vshfl valignbyte vmin %d" % t, {1: rng.integers(0, 64, 64).astype(U32), **({0: a} if a is not None else {})})
    for t in range(128):
        add(B_LANE_RW, "vreadlane vwritelane vlanes vballot lane %d" % (t % 64), r2=t % 64, r3=int(rng.integers(0, 1 << 32)), r4=int(rng.integers(0, 1 << 32)))
    for t in range(100):      # vgather8: every q 0 .. 255 on random tables
        add(B_GATHER, "vgather8 table %d" % t)
    n = len(recs)
    inp = np.zeros((n, 1536), np.uint8)
    inp[:, :1280] = np.array(vecs).reshape(n, 320).view(np.uint8)
    return Launch("C", cfg, np.array(recs), inp, _bwave_out(n, 2048), names=names)


def expect_bwave_lane(L):
    img = L.out.copy()
    mask = np.ones(img.shape, bool)
    O = [img[:, 256 + 256 * k:512 + 256 * k].view(U32) for k in range(4)]
    H = img[:, 256 + 1024:256 + 1024 + 32].view(U32)
    v = L.inp[:, :1280].view(U32).reshape(L.n, 5, 64).astype(np.uint64)
    for i in range(L.n):
        op, r = int(L.rec[i, 0]), L.rec[i]
        a, b, c, d = (v[i, k] for k in range(4))
        if op == B_WALK:
            want = walk_definition(list(L.inp[i, :256]))
            T = len(want)
            for k in (0, 1):
                O[k][i] = M32
                O[k][i, :T] = want
            H[i, :4] = [T, T, 0, 0]
        elif op == B_GATHER:
            img[i, 256:256 + 1024].view(U32)[:] = L.inp[i, :256]
        elif op == B_LANEOPS:
            O[0][i] = ((np.cumsum(a, dtype=np.uint64) - a) & np.uint64(M32)).astype(U32)
            O[1][i] = a[(b & np.uint64(63)).astype(np.int64)].astype(U32)
            O[2][i] = ((((a << np.uint64(32)) | c) >> (np.uint64(8) * (d & np.uint64(3)))) & np.uint64(M32)).astype(U32)
            O[3][i] = np.minimum(a, c).astype(U32)
        else:
            l, s, m = int(r[2]), int(r[3]), int(r[3]) | (int(r[4]) << 32)
            H[i, :4] = [int(a[l]), int(c[l]), 0, 0]
            w = a.copy(); w[l] = s
            O[0][i] = w.astype(U32)
            O[1][i] = [int(a[k]) if (m >> k) & 1 else int(c[k]) for k in range(64)]
            bal = sum((int(a[k]) & 1) << k for k in range(64))
            H[i, 4:8] = [bal & M32, bal >> 32, 0, 0]
    return img, mask


def _disjoint(s, ls, x, lx, kw):
    """[s, s + ls) and [x, x + lx) share no byte of a ring of kw bytes (broadcasting)"""
    return (ls == 0) | (lx == 0) | ((((x - s) % kw) >= ls) & (((s - x) % kw) >= lx))


def _round(rng, kw, tier, odd_round, far_mode, force_len=None):
    """one round of 64 runs: -> (dw, sp, len, mpos, from_stream, gom, farm).  Even lanes literals (from the stream), odd lanes matches
    (from the ring, or far: from memory); destinations disjoint, no source is a destination; lengths legal for the tier; in an odd
    round some lengths are 65 .. 300 (tier 4) and one or two destinations lie at the ring's ends"""
    lo = int(rng.integers(0, 8)) if rng.random() < 0.5 else 0
    hi = 64 - int(rng.integers(0, 8)) if rng.random() < 0.5 else 64
    act = np.zeros(64, bool); act[lo:hi] = True
    top = {0: 15, 1: 31, 4: 64}[tier]
    ln = rng.integers(0, top + 1, 64)
    if tier != 0:      # the tier is the caller's vrun_tier: some run of the round reaches its lower bound
        ln[int(rng.integers(lo, hi))] = int(rng.integers({1: 16, 4: 32}[tier], top + 1))
    if rng.random() < 0.3:
        ln[rng.integers(0, 64, 8)] = rng.choice([0, 1, 2, 3, 4, 7, 8, 15, top], 8)
    ends = []
    if odd_round:
        if tier == 4:
            for l in rng.integers(lo, hi, int(rng.integers(0, 5))):
                ln[l] = int(rng.integers(65, 301))
            ln[rng.integers(lo, hi, 6)] = rng.choice([1, 5, 16, 17, 33, 40, 63, 64, 65, 66], 6)
        ends = list({int(x) for x in rng.integers(lo, hi, int(rng.integers(1, 3)))})
        if tier == 4 and not ends and not (ln[act] > 64).any():
            ends = [lo]
    if force_len is not None:     # every run of the round this long (the step-by-step form's pieces: 16s, then 8 / 4 / 2 / 1)
        ln[:] = force_len
    ln[~act] = 0
    # destinations: in a random order round the ring with random gaps; a reserved stretch over the ring's ends keeps them out of
    # there, an `ends` lane is put there on purpose (rotation)
    order = rng.permutation(np.flatnonzero(act))
    reserve = 0 if ends else 16 + 16 + int(ln.max()) + 1
    seg = np.concatenate([[reserve], ln[order]])
    free = kw - int(seg.sum()) - 8
    assert free > 0
    cuts = np.sort(rng.integers(0, free + 1, len(seg)))
    gaps = np.diff(np.concatenate([[0], cuts]))
    start = np.cumsum(gaps + np.concatenate([[0], seg[:-1]]))
    if ends:
        e = ends[0]
        k = int(np.flatnonzero(order == e)[0]) + 1
        want = int(rng.integers(0, 16)) if rng.random() < 0.5 else kw - int(ln[e]) - 16 + int(rng.integers(1, 16 + int(ln[e])))
        rot = want - int(start[k])
    else:
        rot = (kw - 16 - int(ln.max()) - 1) - int(start[0])
    dw = np.zeros(64, np.int64)
    dw[order] = (start[1:] + rot) % kw
    fs = (np.arange(64) % 2 == 0)
    # sources: stream positions anywhere; ring sources anywhere off every destination (vectorised rejection)
    sp = rng.integers(0, 1 << 20, 64)
    for l in np.flatnonzero(act & ~fs):
        for _ in range(64):
            s = int(rng.integers(0, kw)) if rng.random() < 0.8 else int((kw - rng.integers(0, 80)) % kw)
            if _disjoint(s, int(ln[l]), dw[act], ln[act], kw).all():
                sp[l] = s
                break
        else:
            ln[l] = 0
    gom = sum(1 << int(l) for l in np.flatnonzero(act))
    matches = [int(l) for l in np.flatnonzero(act & ~fs)]
    far = [] if far_mode == 0 or not matches else [matches[int(rng.integers(0, len(matches)))]] if far_mode == 1 else matches
    farm = sum(1 << l for l in far)
    mpos = rng.integers(0, K_FAR - 320, 64)
    dw = dw + kw * rng.integers(0, 4, 64)      # (ring coordinates: the backends mask them)
    return dw, sp, ln, mpos, fs, gom, farm


def bwave_ring_cases(cfg, seed=7, nrounds=300):
    kw, ks = cfg
    rng = np.random.default_rng(seed + kw)
    common = rng.integers(0, 256, ks + kw + K_FAR, dtype=np.uint8)
    recs, vecs, names = [], [], []
    windows = [(0, M32), (1, kw - 1), (2, kw - 130), (130, kw), (kw // 2 + 3, kw // 2 + 255), (255, kw - 253)]   # [lo, hi): a step cut at its first, middle, last dword

    def add(op, name, vec=None, **r):
        rec = np.zeros(REC, U32)
        rec[0] = op
        k = len(recs)
        rec[13], rec[14] = windows[k % len(windows)]
        rec[15] = [0, 4, 1, 255, 77, 128][k % 6]         # wdb: the destination's address mod 256
        for kk, val in r.items():
            rec[int(kk[1:])] = val
        v = rng.integers(0, 1 << 32, (5, 64), dtype=np.uint64).astype(U32)
        for kk, val in (vec or {}).items():
            v[kk] = np.asarray(val).astype(np.uint64).astype(U32)
        recs.append(rec); vecs.append(v); names.append(name)

    ips = list(range(0, 9)) + list(range(ks - 262, ks - 250)) + list(range(ks - 9, ks + 9)) + [int(x) for x in rng.integers(0, 1 << 24, 24)]
    for ip in ips:    # every ip mod 4; windows and per-lane loads that cross the stream ring's end (the 16 mirrored bytes)
        p = rng.integers(0, 1 << 24, 64)
        p[:16] = ks - 8 + np.arange(16) + (ip & ~(ks - 1))
        add(B_WIN, "vs_win vs_ld32 rs_ld64 ip %d" % ip, {1: p}, r2=ip)
    for w in list(range(36)) + list(range(kw - 270, kw)):
        for kind in range(3):
            spos = int(rng.integers(0, K_FAR - 260)) if kind == 2 else int(rng.integers(0, 1 << 20))
            add(B_PUT, "wv_get_%s + wv_put w %d" % (("stream", "ring", "mem")[kind], w), r2=kind, r3=spos, r4=w + kw * int(rng.integers(0, 3)))
    for pred in (0, 1):
        for tier in (0, 1, 4):
            for t in range(nrounds):
                odd_round = t % 3 == 2
                dw, sp, ln, mpos, fs, gom, farm = _round(rng, kw, tier, odd_round, t % 3 if t % 7 else (t // 7) % 3)
                add(B_RUN, "vcopy_run<%d> tier %d round %d%s" % (pred, tier, t, " (ring's ends / long runs)" if odd_round else ""),
                    {0: dw, 1: sp, 2: ln, 3: mpos, 4: fs}, r1=pred, r2=gom & M32, r3=gom >> 32, r4=farm & M32, r5=farm >> 32, r6=tier)
    for ln_ in list(range(1, 41)) + [63, 64, 65, 66]:     # vput through vcopy<0 / 1 / 2>: every run of a step-by-step round this long
        for far_mode in (1, 2):
            dw, sp, ln, mpos, fs, gom, farm = _round(rng, kw, 4, True, far_mode, force_len=ln_)
            add(B_RUN, "vcopy_run step by step, runs of %d bytes" % ln_, {0: dw, 1: sp, 2: ln, 3: mpos, 4: fs}, r1=far_mode & 1, r2=gom & M32,
                r3=gom >> 32, r4=farm & M32, r5=farm >> 32, r6=4)
    n = len(recs)
    inp = np.zeros((n, 1536), np.uint8)
    inp[:, :1280] = np.array(vecs).reshape(n, 320).view(np.uint8)
    return Launch("C", cfg, np.array(recs), inp, _bwave_out(n, 1792 + kw + 256), common=common.tobytes(), names=names)


def expect_bwave_ring(L):
    """a byte-wise model of the two rings: ring[(w + i) mod KW] = source[i]"""
    kw, ks = L.param
    img = L.out.copy()
    mask = np.ones(img.shape, bool)
    common = L.common
    stream, ring0, mem = common[:ks], common[ks:ks + kw], common[ks + kw:]
    O = [img[:, 256 + 256 * k:512 + 256 * k].view(U32) for k in range(4)]
    H = img[:, 256 + 1024:256 + 1024 + 32].view(U32)
    v = L.inp[:, :1280].view(U32).reshape(L.n, 5, 64).astype(np.int64)
    s2 = np.concatenate([stream, stream])
    le32 = lambda by: int.from_bytes(bytes(by), "little")
    for i in range(L.n):
        op, r = int(L.rec[i, 0]), [int(x) for x in L.rec[i][:16]]
        ring = ring0.copy()
        if op == B_WIN:
            ip = r[2]
            for l in range(64):
                q = (ip + 4 * l) % ks
                O[0][i, l], O[1][i, l] = le32(s2[q:q + 4]), le32(s2[q + 4:q + 8])
                q = int(v[i, 1, l]) % ks
                O[2][i, l] = le32(s2[q:q + 4])
            q = ip % ks
            H[i, :4] = [le32(s2[q:q + 4]), le32(s2[q + 4:q + 8]), 0, 0]
            continue
        if op == B_PUT:
            kind, sp, w = r[2], r[3], r[4]
            n = 256 - (w & 3)
            idx = np.arange(n)
            src = stream[(sp + idx) % ks] if kind == 0 else ring[(sp + idx) % kw] if kind == 1 else mem[sp + idx]
            ring[(w + idx) % kw] = src
        else:
            dw, sp, ln, mpos, fs = (v[i, k] for k in range(5))
            gom, farm = r[2] | (r[3] << 32), r[4] | (r[5] << 32)
            new = ring.copy()
            oddm = 0
            for l in range(64):
                x = int(dw[l]) % kw
                if int(ln[l]) > 64 or x < 16 or x + int(ln[l]) + 16 > kw:
                    oddm |= 1 << l
                if not (gom >> l) & 1:
                    continue
                idx = np.arange(int(ln[l]))
                src = stream[(int(sp[l]) + idx) % ks] if fs[l] else mem[int(mpos[l]) + idx] if (farm >> l) & 1 else ring[(int(sp[l]) + idx) % kw]
                new[(int(dw[l]) + idx) % kw] = src
            ring = new
            lens = [int(ln[l]) for l in range(64) if (gom >> l) & 1]
            H[i, :4] = [oddm & M32, oddm >> 32, 4 if any(x >= 32 for x in lens) else 1 if any(x >= 16 for x in lens) else 0, 0]
        ring[kw // 2 + np.arange(16)] = ring[(kw - 1 + np.arange(16)) % kw]      # the probe's observer run
        lo, hi = r[13], min(r[14], kw)
        img[i, 1792 + lo:1792 + hi] = ring[lo:hi]
    return img, mask
