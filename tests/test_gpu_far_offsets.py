"""Every device entry point that takes 64-bit offsets, strides or lengths, at offsets around and past 2^31 and 2^32 -- the table of
tests/far_common.py on the GPU.  One source and one destination far buffer of about 6 GiB each live for the module; the library is
handed views that start behind a red zone of 2^31 + 4096 bytes, so an offset that loses its upper half or is taken for a signed 32-bit
value reads or writes another place of the SAME allocation: a wrong byte, never a fault.  Before every call the whole destination
allocation holds one byte value; afterwards return values and bytes are compared with the reference library's, the blocks' slots are
refilled, and nothing else may be left anywhere in the allocation.  The source holds a non-constant decoy pattern around what is placed.

(The two chain kernels have their test of this kind in test_gpu_cchain.py::test_cchain_device_offsets_past_2_and_4_gib.)"""
import pytest

import far_common as F
from fast_contract_common import DECODE_VARIANTS, DEFAULT_KNOBS, set_knobs

pytestmark = pytest.mark.gpu
FILLS = (0x5A, 0xC3, 0x00, 0xFF)


@pytest.fixture(scope="module")
def far(amd):
    import torch
    fb = F.FarBuffers(torch, torch.device("cuda", 0))
    yield fb
    fb.free()
    del fb
    torch.cuda.empty_cache()


def launch(fb, slots, call, fill):
    """one launch of the common shape call(src, src_off, src_len, dst, dst_off, p1, out) over the placed slots -> the return values"""
    torch = fb.torch
    out = torch.full((len(slots),), -12345, dtype=torch.int32, device=fb.dev)
    fb.fill(fill)
    call(fb.src, fb.i64([s.src_at for s in slots]), fb.i32([len(s.data) for s in slots]), fb.dst,
         fb.i64([s.dst_at for s in slots]), fb.i32([s.p1 for s in slots]), out)
    torch.cuda.synchronize()
    return out.cpu().tolist()


def launch2(fb, slots, call, fill):
    """the destSize shape: call(src, src_off, src_len, dst, dst_off, target, out, consumed) -> (return values, consumed)"""
    torch = fb.torch
    out = torch.full((len(slots),), -12345, dtype=torch.int32, device=fb.dev)
    cons = torch.full((len(slots),), -12345, dtype=torch.int32, device=fb.dev)
    fb.fill(fill)
    call(fb.src, fb.i64([s.src_at for s in slots]), fb.i32([len(s.data) for s in slots]), fb.dst, fb.i64([s.dst_at for s in slots]),
         fb.i32([s.p1 for s in slots]), out, cons)
    torch.cuda.synchronize()
    return out.cpu().tolist(), cons.cpu().tolist()


def test_far_compress_fast(amd, ref, corpus, far):
    """the three cores and, for the blocks of 65547 bytes and more, packed and 64-bit table entries; full, exact and size - 1 capacities"""
    slots = F.compress_fast_cases(ref, corpus)
    far.put(slots)
    try:
        k = 0
        for core in (1, 3, 5):
            for pack in (1, 0):
                amd.set_option("compress_core", core)
                amd.set_option("compress_pack", pack)
                fill = FILLS[k % 4]; k += 1
                far.settle(slots, launch(far, slots, amd.DeviceBatch.compress_fast, fill), fill, ("compress_fast", "core", core, "pack", pack))
    finally:
        amd.set_option("compress_core", 5)
        amd.set_option("compress_pack", 1)


def test_far_compress_accel(amd, ref, corpus, far):
    for k, a in enumerate((2, 64)):
        slots = F.compress_accel_cases(ref, corpus, a)
        far.put(slots)
        rets = launch(far, slots, lambda *t: amd.DeviceBatch.compress_fast(*t, acceleration=a), FILLS[k])
        far.settle(slots, rets, FILLS[k], ("acceleration", a))


def test_far_compress_dest_size(amd, ref, corpus, far):
    slots = F.dest_size_cases(ref, corpus)
    far.put(slots)
    rets, cons = launch2(far, slots, amd.DeviceBatch.compress_dest_size, 0x5A)
    far.settle(slots, rets, 0x5A, "compress_dest_size", ret2=cons)


def test_far_compress_hc(amd, ref, corpus, far):
    """both forms: the workspace of one u16 per source byte is indexed by the block's source offset, so with src_span = SPAN it is
    about 8 GiB and its far end is used; the plain form sizes the same workspace itself"""
    import torch
    for k, level in enumerate((1, 9, 12)):
        slots = F.compress_hc_cases(ref, corpus, level)
        far.put(slots)
        assert far.src.numel() == F.SPAN and amd.lib().lz4hip_hc_workspace_bytes(F.SPAN, len(slots), level) >= 2 * F.SPAN
        rets = launch(far, slots, lambda *t: amd.DeviceBatch.compress_hc(*t, level=level), FILLS[k])
        far.settle(slots, rets, FILLS[k], ("compress_hc, caller's workspace", level))
        torch.cuda.empty_cache()          # (the workspace goes back before the library allocates its own)
        rets = launch(far, slots, lambda *t: amd.DeviceBatch.compress_hc_sync(*t, level=level), FILLS[k + 1])
        far.settle(slots, rets, FILLS[k + 1], ("compress_hc, own workspace", level))


def test_far_compress_hc_dest_size(amd, ref, corpus, far):
    import torch
    for k, level in enumerate((4, 9)):
        slots = F.hc_dest_size_cases(ref, corpus, level)
        far.put(slots)
        rets, cons = launch2(far, slots, lambda *t: amd.DeviceBatch.compress_hc_dest_size(*t, level=level), FILLS[k])
        far.settle(slots, rets, FILLS[k], ("compress_hc_dest_size, caller's workspace", level), ret2=cons)
        torch.cuda.empty_cache()
        rets, cons = launch2(far, slots, lambda *t: amd.DeviceBatch.compress_hc_dest_size_sync(*t, level=level), FILLS[k + 2])
        far.settle(slots, rets, FILLS[k + 2], ("compress_hc_dest_size, own workspace", level), ret2=cons)


def test_far_dictionary(amd, ref, far):
    """the four dictionary entry points against a 4 KiB and a 64 KiB dictionary"""
    import torch
    for L in F.DICT_LENS:
        d = F.dict_of(L)
        dic = amd.LZ4Dictionary(d)
        try:
            slots = F.compress_dict_cases(ref, L)
            far.put(slots)
            rets = launch(far, slots, lambda *t: amd.DeviceBatch.compress_dict(*t, dic), 0x5A)
            far.settle(slots, rets, 0x5A, ("compress_dict", L))
            slots = F.compress_hc_dict_cases(ref, L)
            far.put(slots)
            rets = launch(far, slots, lambda *t: amd.DeviceBatch.compress_hc_dict(*t, dic, level=9), 0xC3)
            far.settle(slots, rets, 0xC3, ("compress_hc_dict, caller's workspace", L))
            torch.cuda.empty_cache()
            rets = launch(far, slots, lambda *t: amd.DeviceBatch.compress_hc_dict_sync(*t, dic, level=9), 0x00)
            far.settle(slots, rets, 0x00, ("compress_hc_dict, own workspace", L))
            slots = F.decode_dict_cases(ref, L)
            far.put(slots)
            d_dev = far.up(d)
            rets = launch(far, slots, lambda *t: amd.DeviceBatch.decompress_safe_dict(*t, d_dev), 0xFF)
            far.settle(slots, rets, 0xFF, ("decompress_safe_dict", L))
        finally:
            torch.cuda.synchronize()
            dic.close()


def test_far_decode_variants(amd, ref, O, corpus, far):
    """every decoder kernel the knobs can select, over one placed batch of valid and damaged streams"""
    slots = F.decode_safe_cases(ref, O, corpus)
    far.put(slots)
    try:
        for k, knobs in enumerate(DECODE_VARIANTS):
            set_knobs(amd, knobs)
            fill = FILLS[k % 4]
            far.settle(slots, launch(far, slots, amd.DeviceBatch.decompress_safe, fill), fill, ("decompress_safe", knobs))
    finally:
        set_knobs(amd, DEFAULT_KNOBS)


def test_far_decode_routed(amd, ref, O, corpus, far):
    """more than 16 blocks per CU: decode_route_kernel chooses the loop on the device, from the sizes of 64 streams and the middle of 32.
    Text slices and App. F blocks, streams and outputs each laid out back to back across 2^32, then across 2^31 -- as 1 KiB blocks,
    whose streams are too short to be sampled (the kernel reads src_len and nothing else), and as 16 KiB blocks, whose streams it
    samples.  That the launch was routed: last_decode_route holds the average of THIS batch's 64 sampled sizes, and sampled sequences
    where there is something to sample"""
    import torch
    n = 16 * torch.cuda.get_device_properties(0).multi_processor_count + 64
    k = 0
    for size in F.ROUTED_SIZES:
        made = {kind: F.routed_streams(ref, O, corpus, kind, n, size) for kind in ("text", "appf")}
        for boundary in (F.B32, F.B31):
            for kind in ("text", "appf"):
                streams, blocks = made[kind]
                blob, want = b"".join(streams), b"".join(blocks)
                s_at, d_at = F.routed_place(boundary, len(blob)), F.routed_place(boundary, len(want))
                assert s_at < boundary < s_at + len(blob) and d_at < boundary < d_at + len(want)
                offs, p = [], s_at
                for s in streams:
                    offs.append(p); p += len(s)
                lens = [len(s) for s in streams]
                far.src[s_at:s_at + len(blob)] = far.up(blob)
                out = torch.full((n,), -12345, dtype=torch.int32, device=far.dev)
                fill = FILLS[k % 4]; k += 1
                far.fill(fill)
                amd.DeviceBatch.decompress_safe(far.src, far.i64(offs), far.i32(lens), far.dst, far.i64([d_at + size * i for i in range(n)]),
                                                far.i32([size] * n), out)
                torch.cuda.synchronize()
                route = amd.last_decode_route()
                assert route[3] == sum(lens[i * (n // 64)] for i in range(64)) // 64, ("the launch was not routed", kind, size, boundary, route)
                assert min(lens) >= 4096 if size > 1024 else max(lens) < 4096    # (streams under 4 KiB are not sampled)
                assert (route[5] > 0 and route[2] > 0) == (size > 1024), ("the sampler", kind, size, boundary, route)
                assert out.cpu().tolist() == [size] * n, (kind, size, boundary)
                assert far.get(d_at, len(want)) == want, (kind, size, boundary, "bytes differ")
                far.dst[d_at:d_at + len(want)] = fill
                assert far.untouched(far.dst_all, fill) == 0, (kind, size, boundary, "bytes written outside the slots")


def test_far_decode_fast_partial_size(amd, ref, O, corpus, far):
    import torch
    from partial_common import same_bytes
    slots = F.decode_fast_cases(ref, O, corpus)
    far.put(slots)
    far.settle(slots, launch(far, slots, amd.DeviceBatch.decompress_fast, 0x5A), 0x5A, "decompress_fast")

    slots = F.decode_partial_cases(ref, O, corpus)
    far.put(slots)
    out = torch.full((len(slots),), -12345, dtype=torch.int32, device=far.dev)
    far.fill(0xC3)
    amd.DeviceBatch.decompress_safe_partial(far.src, far.i64([s.src_at for s in slots]), far.i32([len(s.data) for s in slots]), far.dst,
                                            far.i64([s.dst_at for s in slots]), far.i32([s.p1 for s in slots]), far.i32([s.p2 for s in slots]), out)
    torch.cuda.synchronize()
    # (a cut match of offset 0 -- only a damaged stream has one -- is the one place where liblz4's bytes are not defined)
    far.settle(slots, out.cpu().tolist(), 0xC3, "decompress_safe_partial", same=lambda s, got: same_bytes(got, s.out, s.data, s.ret, min(s.p1, s.p2)))

    slots = F.decode_size_cases(ref, O, corpus)
    far.put(slots)
    out = torch.full((len(slots),), -12345, dtype=torch.int32, device=far.dev)
    far.fill(0x00)
    amd.DeviceBatch.decoded_size(far.src, far.i64([s.src_at for s in slots]), far.i32([len(s.data) for s in slots]), far.i32([s.p1 for s in slots]), out)
    torch.cuda.synchronize()
    far.settle(slots, out.cpu().tolist(), 0x00, "decoded_size")


def test_far_xxh(amd, ref, far):
    """both kernels of XXH32 and XXH64: the wave-per-buffer kernels (at most 512 buffers) on a few long buffers at every place, the
    lane-group kernels on 600 short ones laid out across 2^32; two seeds"""
    import torch
    slots = F.xxh_long_cases()
    img, at, off, lens = F.xxh_short_layout()
    batches = [("long", [s.src_at for s in slots], [len(s.data) for s in slots], [s.data for s in slots]),
               ("short", off, lens, [img[o - at:o - at + n] for o, n in zip(off, lens)])]
    for what, offs, ln, datas in batches:
        assert (len(offs) <= 512) == (what == "long")
        if what == "long":
            far.put(slots)
        else:                                      # (over the long buffer that lay across 2^32)
            far.src[at:at + len(img)] = far.up(img)
        o_t, l_t = far.i64(offs), far.i32(ln)
        for seed in F.XXH_SEEDS:
            o32 = torch.zeros(len(offs), dtype=torch.int32, device=far.dev)
            o64 = torch.zeros(len(offs), dtype=torch.int64, device=far.dev)
            amd.DeviceBatch.xxh32(far.src, o_t, l_t, seed, o32)
            amd.DeviceBatch.xxh64(far.src, o_t, l_t, seed, o64)
            torch.cuda.synchronize()
            a, b = o32.cpu().tolist(), o64.cpu().tolist()
            bad = [(what, seed, i, offs[i], ln[i]) for i, v in enumerate(datas)
                   if a[i] & 0xFFFFFFFF != ref.xxh32(v, seed) or b[i] & 0xFFFFFFFFFFFFFFFF != ref.xxh64(v, seed)]
            assert not bad, (len(bad), bad[:4])


def test_far_gen_blocks(amd, O, far):
    """stride * index passes 2^32 inside the kernel: 70 blocks of 1000 bytes, 2^26 apart, from the start of the destination allocation
    (70 strides do not fit behind the red zone)"""
    import torch
    far.fill(0x5A)
    amd.DeviceBatch.gen_blocks(far.dst_all, F.GEN_STRIDE, F.GEN_LEN, F.GEN_BLOCKS, first_idx=5)
    torch.cuda.synchronize()
    bad = [i for i in range(F.GEN_BLOCKS) if far.get(i * F.GEN_STRIDE, F.GEN_LEN, far.dst_all) != O.gen_block(F.GEN_LEN, 5 + i)]
    assert not bad, bad
    for i in range(F.GEN_BLOCKS):
        far.dst_all[i * F.GEN_STRIDE:i * F.GEN_STRIDE + F.GEN_LEN] = 0x5A
    assert far.untouched(far.dst_all, 0x5A) == 0


@pytest.mark.parametrize("data", sorted(F.CONTAINER_INPUTS))
def test_far_containers(amd, ref, O, far, data):
    """the container writer and reader take lengths, not offsets: 1030 blocks of 4 MiB generated on the device.  "appf": App. F data,
    ratio 2 -- the input, the writer's compressed slots and the reader's output slots pass 2^32, the container does not.  "dense":
    1000 blocks of long literal runs (stored raw) and 30 that just compress (ratio 1.02) -- the CONTAINER passes 2^32 as well, inside the
    compressed blocks: the writer's scan, header and payload offsets, the checksum pass and the reader's walk all form offsets past it.
    Kinds 0 (with block checksums) and 1: the total; header, payload and checksum of the first and last block, of the two blocks on
    either side of input offset 2^32 and of the two on either side of OUTPUT offset 2^32 (where there is one) against the reference
    compressor and ref.xxh32; nothing written behind the total; and the device round trip back to the input"""
    import torch
    n, blk = F.CONTAINER_BLOCKS, F.CONTAINER_BLOCK
    nbytes, first = n * blk, 7 << 20
    src = far.src_all[:nbytes]
    L = amd.lib()
    parts = F.CONTAINER_INPUTS[data]
    assert sum(cnt for cnt, _ in parts) == n

    def params(k):
        b0 = 0
        for cnt, kw in parts:
            if k < b0 + cnt:
                return kw
            b0 += cnt

    def want_block(kind, v):
        """what the reference writers emit for the block v (LZ4FrameOutputStream.writeBlock / LZ4BlockOutputStream.flushBufferedData)"""
        c = ref.compress_fast(v)
        raw = len(c) >= len(v)
        pay = v if raw else c
        if kind == 0:
            return (len(pay) | (0x80000000 if raw else 0)).to_bytes(4, "little") + pay + ref.xxh32(pay, 0).to_bytes(4, "little")
        return (b"LZ4Block" + bytes([(0x10 if raw else 0x20) | 12]) + len(pay).to_bytes(4, "little") + len(v).to_bytes(4, "little")
                + (ref.xxh32(v, 0x9747b28c) & 0x0FFFFFFF).to_bytes(4, "little") + pay)

    try:
        b0 = 0
        for cnt, kw in parts:
            amd.DeviceBatch.gen_blocks(src[b0 * blk:], blk, blk, cnt, first_idx=first + b0, **kw)
            b0 += cnt
        torch.cuda.synchronize()
        host = {}

        def block(k):
            if k not in host:
                host[k] = far.get(k * blk, blk, src)
                assert host[k] == O.gen_block(blk, first + k, **params(k)), ("generated block", k)
            return host[k]

        back = torch.empty(nbytes, dtype=torch.uint8, device=far.dev)
        wsb = L.lz4hip_container_decode_workspace_bytes(n)
        ws = torch.empty(wsb, dtype=torch.uint8, device=far.dev)
        sizes = torch.zeros(n, dtype=torch.int32, device=far.dev)
        info = torch.zeros(5, dtype=torch.int64, device=far.dev)
        total = torch.zeros(1, dtype=torch.int64, device=far.dev)
        for kind in (0, 1):
            far.fill(0xE7)
            amd.DeviceBatch.container_blocks(kind, src, blk, far.dst_all, total, block_checksum=(kind == 0))
            torch.cuda.synchronize()
            tot = int(total.item())
            pos, where = 0, {}
            for k in range(n):          # the walk over the size words / headers
                if kind == 0:
                    ln = 4 + (int.from_bytes(far.get(pos, 4, far.dst_all), "little") & 0x7FFFFFFF) + 4
                else:
                    ln = 21 + int.from_bytes(far.get(pos + 9, 4, far.dst_all), "little")
                where[k] = (pos, ln)
                pos += ln
                assert pos <= tot, (data, kind, k, pos, tot)
            assert pos == tot, (data, kind, pos, tot)
            probe = [0, F.B32 // blk - 1, F.B32 // blk, n - 1]
            assert (tot > F.B32) == (data == "dense"), (data, kind, tot)
            if tot > F.B32:
                k1 = max(k for k in range(n) if where[k][0] < F.B32)       # the block that holds or ends at output offset 2^32
                assert k1 + 1 < n and where[k1][1] < blk and where[k1 + 1][1] < blk, (data, kind, "compressed blocks on either side", k1)
                probe += [k1 - 1, k1, k1 + 1, parts[0][0] - 1]
            for k in probe:
                want = want_block(kind, block(k))
                assert where[k][1] == len(want) and far.get(where[k][0], len(want), far.dst_all) == want, (data, kind, "block", k, where[k])
            far.dst_all[:tot] = 0xE7
            assert far.untouched(far.dst_all, 0xE7) == 0, (data, kind, "bytes written behind the total")
            # the round trip: block k decodes to back + k * blk
            amd.DeviceBatch.container_blocks(kind, src, blk, far.dst_all, total, block_checksum=(kind == 0))
            back.zero_()
            rc = L.lz4hip_container_decode_dev(kind, 1 if kind == 0 else 0, far.dst_all.data_ptr(), tot, blk, back.data_ptr(), blk, n, sizes.data_ptr(),
                                               info.data_ptr(), ws.data_ptr(), wsb, 0, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert rc == 0, L.lz4hip_last_error()
            assert [int(x) for x in info[:4].cpu()] == [n, tot, 1, nbytes], (data, kind, info.cpu().tolist())
            assert bool((sizes == blk).all()) and torch.equal(back, src), (data, kind, "round trip")
    finally:
        torch.cuda.synchronize()
        back = ws = None
        torch.cuda.empty_cache()
        far.decoy(far.src_all)
