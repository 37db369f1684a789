"""Ranged decode on the GPU: blocks [firstBlock, firstBlock + numBlocks) of an archive, without the rest.

Everything is bit-exact: the expected output is the corresponding slice of the original input (the lossless round
trip), and in the same test it must equal the slice of the existing whole-element decode.  Element sizes are the class
and tile boundaries of the decoder's geometry (4096 x {1, 2, 3, 4, 5, 8, 9, 16, 17, 33}, with and without a partial
last block); every output buffer sits between 64 guard bytes that must not change.  Status and size follow the contract
of include/dietgpu_amd.h: success needs firstBlock * 4096 <= total and the clipped range inside the capacity, and
outSize = min(total, (firstBlock + numBlocks) * 4096) - firstBlock * 4096.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BLK = 4096
U32_MAX = 0xFFFFFFFF
GUARD = 64  # bytes on both sides of every output
FT_DTYPE = {0: torch.uint8, O.FLOAT16: torch.float16, O.BFLOAT16: torch.bfloat16, O.FLOAT32: torch.float32}
WORD_DTYPE = {0: torch.uint8, O.FLOAT16: torch.int16, O.BFLOAT16: torch.int16, O.FLOAT32: torch.int32}
WORD_BYTES = {0: 1, O.FLOAT16: 2, O.BFLOAT16: 2, O.FLOAT32: 4}
TYPES = [0, O.FLOAT16, O.BFLOAT16, O.FLOAT32]
SIZES = [BLK * k + extra for k in (1, 2, 3, 4, 5, 8, 9, 16, 17, 33) for extra in (0, 1234)]
ROUTES = ["torch_ops", "ctypes", "cabi"]


@pytest.fixture(scope="module")
def dg():
    import dietgpu_amd

    dietgpu_amd.lib()  # fails loudly if the HIP extension is missing
    dietgpu_amd.load_torch_ops()
    yield dietgpu_amd
    dietgpu_amd.prefer_torch_ops(True)


def make_words(ft, n, seed):
    """numpy words of the archive's type: skewed bytes, or N(0, 1) in the float format"""
    rng = np.random.default_rng(seed)
    if ft == 0:
        return np.minimum(rng.exponential(12.0, n), 255).astype(np.uint8)
    f = rng.standard_normal(n).astype(np.float32)
    if ft == O.FLOAT16:
        return f.astype(np.float16).view(np.uint16)
    if ft == O.BFLOAT16:
        return (f.view(np.uint32) >> 16).astype(np.uint16)
    return f.view(np.uint32).copy()


def to_tensor(ft, w):
    if ft == 0:
        return torch.from_numpy(w.copy()).to(DEV)
    return torch.from_numpy(w.view(np.int16 if w.dtype == np.uint16 else np.int32).copy()).to(DEV).view(FT_DTYPE[ft])


def as_words(ft, t):
    return t.view(WORD_DTYPE[ft])


def gpu_archives(dg, ft, xs, p):
    comp, sizes, _ = dg.compress_data(ft != 0, xs, False, None, prob_bits=p)
    return [comp[i, :n].clone() for i, n in enumerate(sizes.tolist())]


def full_decode(dg, ft, archs, xs, p):
    outs = [torch.empty_like(x) for x in xs]
    status = torch.zeros((len(xs),), dtype=torch.uint8, device=DEV)
    dg.decompress_data(ft != 0, archs, outs, False, None, status, None, prob_bits=p)
    assert status.cpu().numpy().all()
    for o, x in zip(outs, xs):
        assert torch.equal(as_words(ft, o), as_words(ft, x))
    return outs


def expected(total, first, count, cap=None):
    """(status, outSize, words written) of a ranged decode, from the contract"""
    if count == 0:
        return 1, 0, 0
    lo = first * BLK
    if lo > total:
        return 0, 0, 0
    size = min(total, (first + count) * BLK) - lo
    if cap is not None and size > cap:
        return 0, size, 0
    return 1, size, size


# the kinds of range every batch is decoded with, as (first, count) of an element of `total` words in `nb` blocks
KINDS = {
    "first block": lambda nb, total: (0, 1),
    "last block": lambda nb, total: (nb - 1, 1),
    "odd first, even count": lambda nb, total: (1, 2),
    "even first, odd count": lambda nb, total: (2, 3),
    # tiles are counted from the range's first block: 20 blocks from block 3 are two 16-block tiles (five 4-block ones
    # in a call whose largest range is small), on elements that have them; clipped or rejected on the shorter ones
    "across a 16-block tile edge": lambda nb, total: (3, 20),
    "across a 4-block tile edge": lambda nb, total: (1, 6),
    "whole element": lambda nb, total: (0, nb),
    "to the end": lambda nb, total: (min(1, nb - 1), U32_MAX),
    "no blocks": lambda nb, total: (1, 0),
    "first at the end": lambda nb, total: (nb, 1),
    "first past the end": lambda nb, total: (nb + 1, 1),
}


class Outputs:
    """One guarded output buffer per element: [GUARD bytes | shift | range | GUARD bytes], all 0xA5 before the call."""

    def __init__(self, ft, wants, shift_bytes=0):
        self.ft, self.wb = ft, WORD_BYTES[ft]
        self.g = (GUARD + shift_bytes) // self.wb
        self.bufs = [torch.full(((2 * self.g + w) * self.wb,), 0xA5, dtype=torch.uint8, device=DEV).view(WORD_DTYPE[ft]) for w in wants]
        self.wants = wants
        self.outs = [b[self.g : self.g + w].view(FT_DTYPE[ft]) for b, w in zip(self.bufs, wants)]
        self.fresh = [b.clone() for b in self.bufs]
        if shift_bytes:
            assert all(o.data_ptr() % 16 != 0 and o.data_ptr() % self.wb == 0 for o in self.outs if o.numel())

    def check(self, i, written, want_words):
        """the first `written` words equal want_words, everything else -- guards included -- is untouched"""
        buf, fresh, g = self.bufs[i], self.fresh[i], self.g
        assert torch.equal(buf[:g], fresh[:g]), "front guard"
        assert torch.equal(buf[g + written :], fresh[g + written :]), "tail / rear guard"
        if written:
            assert torch.equal(buf[g : g + written], want_words)


def call_range(dg, route, ft, p, archs, outs, first, count, status, osz, temp=None):
    """the block-granular call on one of the three routes -> temp bytes used"""
    if route == "cabi":
        L = dg.lib()
        n = len(archs)
        ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        u32s = lambda vs: (C.c_uint32 * n)(*vs)
        caps = [o.numel() for o in outs]
        in_bytes = [a.numel() for a in archs]
        used = C.c_size_t(12345)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        tp, tb = (C.c_void_p(temp.data_ptr()), temp.numel()) if temp is not None else (None, 0)
        if ft:
            rc = L.dgpu_float_decompress_range(tp, tb, C.byref(used), ft, p, n, ptrs(archs), u32s(in_bytes), u32s(first), u32s(count),
                                               ptrs(outs), u32s(caps), C.c_void_p(status.data_ptr()), C.c_void_p(osz.data_ptr()), st)
        else:
            rc = L.dgpu_ans_decode_batch_pointer_range(tp, tb, C.byref(used), p, n, ptrs(archs), u32s(in_bytes), u32s(first),
                                                       u32s(count), ptrs(outs), u32s(caps), C.c_void_p(status.data_ptr()),
                                                       C.c_void_p(osz.data_ptr()), st)
        assert rc == 0, L.dgpu_last_error()
        return used.value
    dg.prefer_torch_ops(route == "torch_ops")
    try:
        return dg.decompress_data_range(ft != 0, archs, outs, first, count, temp, status, osz, prob_bits=p)
    finally:
        dg.prefer_torch_ops(True)


def run_and_check(dg, route, ft, p, archs, xs, fulls, ranges, shift_bytes=0):
    """one ranged call for the batch; every element against the input, the whole decode and the contract"""
    totals = [x.numel() for x in xs]
    exp = [expected(t, f, c) for t, (f, c) in zip(totals, ranges)]
    wants = [e[1] for e in exp]
    o = Outputs(ft, wants, shift_bytes)
    status = torch.full((len(xs),), 7, dtype=torch.uint8, device=DEV)
    osz = torch.full((len(xs),), -7, dtype=torch.int32, device=DEV)
    used = call_range(dg, route, ft, p, archs, o.outs, [r[0] for r in ranges], [r[1] for r in ranges], status, osz)
    advertised = (dg.lib().dgpu_float_decompress_temp_bytes(ft, len(xs), max(totals), p) if ft
                  else dg.lib().dgpu_ans_decode_temp_bytes(len(xs), max(totals), p))
    assert used <= advertised
    hs, hz = status.tolist(), osz.tolist()
    for i, ((st, size, written), (first, count)) in enumerate(zip(exp, ranges)):
        what = f"{route} ft={ft} p={p} total={totals[i]} first={first} count={count}"
        assert hs[i] == st, what
        assert hz[i] == size, what
        lo = first * BLK
        want = as_words(ft, xs[i])[lo : lo + written]
        if written:
            assert torch.equal(want, as_words(ft, fulls[i])[lo : lo + written]), what  # = the slice of the whole decode
        o.check(i, written, want)


@pytest.mark.parametrize("p", [9, 10, 11])
@pytest.mark.parametrize("ft", TYPES)
def test_ranges_of_batches_of_one_size(dg, ft, p):
    for si, total in enumerate(SIZES):
        xs = [to_tensor(ft, make_words(ft, total, 1000 * si + j)) for j in range(2)]
        archs = gpu_archives(dg, ft, xs, p)
        fulls = full_decode(dg, ft, archs, xs, p)
        nb = (total + BLK - 1) // BLK
        for name, kind in KINDS.items():
            for route in ("torch_ops", "ctypes"):
                run_and_check(dg, route, ft, p, archs, xs, fulls, [kind(nb, total)] * 2)


@pytest.mark.parametrize("p", [9, 10, 11])
@pytest.mark.parametrize("ft", TYPES)
def test_ranges_of_a_mixed_batch(dg, ft, p):
    """all twenty sizes in one call (one geometry, from the largest range), outputs word-aligned but not 16-byte
    aligned, every kind of range -- the same kind for every element, then a different kind for each"""
    xs = [to_tensor(ft, make_words(ft, total, 77 + i)) for i, total in enumerate(SIZES)]
    archs = gpu_archives(dg, ft, xs, p)
    fulls = full_decode(dg, ft, archs, xs, p)
    nbs = [(t + BLK - 1) // BLK for t in SIZES]
    shift = 4  # bytes: one fp32 word, two 16-bit words, the alignment raw ANS data needs
    kinds = list(KINDS.values())
    for route in ROUTES:
        for kind in kinds:
            run_and_check(dg, route, ft, p, archs, xs, fulls, [kind(nb, t) for nb, t in zip(nbs, SIZES)], shift)
        assorted = [kinds[(i + 3) % len(kinds)](nb, t) for i, (nb, t) in enumerate(zip(nbs, SIZES))]
        run_and_check(dg, route, ft, p, archs, xs, fulls, assorted, shift)
        run_and_check(dg, route, ft, p, archs, xs, fulls, assorted, 0)
        # small ranges only: the 4-block geometry on elements of up to 33 blocks
        small = [(min(nb - 1, 1 + i % 3), 1 + i % 5) for i, nb in enumerate(nbs)]
        run_and_check(dg, route, ft, p, archs, xs, fulls, small, shift)


@pytest.mark.parametrize("ft", TYPES)
def test_ranges_of_oracle_archives(dg, ft):
    """the archives come from the CPU oracle, not from the encoder under test"""
    sizes = [BLK * 5 + 1234, BLK * 17, BLK * 2]
    for p in (9, 10, 11):
        ws = [make_words(ft, n, 31 * p + i) for i, n in enumerate(sizes)]
        xs = [to_tensor(ft, w) for w in ws]
        archs = [torch.from_numpy((O.float_compress(ft, w, p) if ft else O.ans_encode(w, p)).copy()).to(DEV) for w in ws]
        fulls = full_decode(dg, ft, archs, xs, p)
        nbs = [(t + BLK - 1) // BLK for t in sizes]
        for kind in KINDS.values():
            for route in ROUTES:
                run_and_check(dg, route, ft, p, archs, xs, fulls, [kind(nb, t) for nb, t in zip(nbs, sizes)], 4)


@pytest.mark.parametrize("ft", [O.FLOAT16, O.BFLOAT16, O.FLOAT32])
def test_ranges_of_floats_on_both_staging_modes(dg, ft):
    """make_words gives every float type one staging mode (N(0, 1): fp16 blocks always take the word ring, bf16 and fp32
    blocks never).  The elements of tests/accum_cases.py hold, for every type, waves staged whole, ring waves, waves that
    mix the two, and 24 blocks at the 1024-word limit (tests/test_accumulate_cases_host.py asserts it on these archives)."""
    import accum_cases as AC

    case = AC.staging(ft, 0)
    members = [AC.STAGING_MIXED, AC.STAGING_BOUNDARY]
    ws = [case.words[i] for i in members]
    sizes = [w.size for w in ws]
    xs = [to_tensor(ft, w) for w in ws]
    archs = [torch.from_numpy(case.archives(10)[i].copy()).to(DEV) for i in members]
    fulls = full_decode(dg, ft, archs, xs, 10)
    nbs = [(t + BLK - 1) // BLK for t in sizes]
    for kind in KINDS.values():
        for route in ROUTES:
            for shift in (0, 4):
                run_and_check(dg, route, ft, 10, archs, xs, fulls, [kind(nb, t) for nb, t in zip(nbs, sizes)], shift)


@pytest.mark.parametrize("ft", TYPES)
def test_a_range_that_does_not_fit_its_buffer_is_reported(dg, ft):
    total = BLK * 9 + 1234
    xs = [to_tensor(ft, make_words(ft, total, 5 + j)) for j in range(2)]
    archs = gpu_archives(dg, ft, xs, 10)
    for route in ROUTES:
        o = Outputs(ft, [3 * BLK - 1, 3 * BLK])
        status = torch.full((2,), 7, dtype=torch.uint8, device=DEV)
        osz = torch.zeros((2,), dtype=torch.int32, device=DEV)
        call_range(dg, route, ft, 10, archs, o.outs, [4, 4], [3, 3], status, osz)
        assert status.tolist() == [0, 1] and osz.tolist() == [3 * BLK, 3 * BLK]  # the size needed is reported
        o.check(0, 0, None)
        o.check(1, 3 * BLK, as_words(ft, xs[1])[4 * BLK : 7 * BLK])


def _corrupt(arch, offset, value):
    bad = arch.copy()
    bad[offset : offset + 4].view(np.uint32)[0] = value
    return torch.from_numpy(bad).to(DEV)


@pytest.mark.parametrize("ft", [0, O.BFLOAT16])
def test_range_decoder_rejects_malformed_archives(dg, ft):
    """deterministic corruptions of an oracle archive (as test_decoder_rejects_*): a descriptor inside the range fails
    the call and its block is not written; the same corruption outside the range is not even looked at"""
    nb, total = 6, 5 * BLK + 100
    w = make_words(ft, total, 9)
    x = to_tensor(ft, w)
    good = O.float_compress(ft, w, 10) if ft else O.ans_encode(w, 10)
    ans = 16 + O.float_uncomp_data_size(ft, total) if ft else 0  # the ANS archive inside a float archive
    bw0 = ans + 32 + 512 + 128 * nb  # the block descriptors {uncompressed << 16 | compressed words, start}
    u32 = lambda off: int(good[off : off + 4].view(np.uint32)[0])
    cases = [
        ("block 2: uncompressed size", bw0 + 2 * 8, (4095 << 16) | (u32(bw0 + 2 * 8) & 0xFFFF)),
        ("block 2: start past the end", bw0 + 2 * 8 + 4, u32(ans + 12)),
        ("block 2: start unaligned", bw0 + 2 * 8 + 4, u32(bw0 + 2 * 8 + 4) + 3),
    ]
    for route in ROUTES:
        for name, off, val in cases:
            bad = _corrupt(good, off, val)
            for (first, count), want_status in (((1, 3), 0), ((2, 1), 0), ((3, 3), 1), ((0, 2), 1), ((3, U32_MAX), 1)):
                st, size, written = expected(total, first, count)
                o = Outputs(ft, [size])
                status = torch.full((1,), 7, dtype=torch.uint8, device=DEV)
                osz = torch.zeros((1,), dtype=torch.int32, device=DEV)
                call_range(dg, route, ft, 10, [bad], o.outs, [first], [count], status, osz)
                torch.cuda.synchronize()
                assert status.item() == want_status, (route, name, first, count)
                lo = first * BLK
                if want_status:
                    o.check(0, size, as_words(ft, x)[lo : lo + size])
                else:
                    # guards untouched, and the words of the malformed block are as they were
                    g, b2 = o.g, (2 - first) * BLK
                    assert torch.equal(o.bufs[0][:g], o.fresh[0][:g]) and torch.equal(o.bufs[0][g + size :], o.fresh[0][g + size :])
                    assert torch.equal(o.bufs[0][g + b2 : g + b2 + BLK], o.fresh[0][g + b2 : g + b2 + BLK]), (route, name)
        # header corruptions fail a ranged call as they fail a whole decode
        header = [("magic", ans + 0, 0xD00D0002), ("numBlocks", ans + 4, nb + 1), ("total", ans + 8, total - 200), ("probBits", ans + 16, 11)]
        if ft:
            header += [("float magic", 0, 0xF00F0003), ("float type", 8, O.FLOAT16), ("float size", 4, total - 16)]
        for name, off, val in header:
            o = Outputs(ft, [2 * BLK])
            status = torch.full((1,), 7, dtype=torch.uint8, device=DEV)
            call_range(dg, route, ft, 10, [_corrupt(good, off, val)], o.outs, [1], [2], status, torch.zeros((1,), dtype=torch.int32, device=DEV))
            assert status.item() == 0, (route, name)
            o.check(0, 0, None)
        # inBytes below the archive's size: the tensor is cut short
        garch = torch.from_numpy(good.copy()).to(DEV)
        for cut in (8, 31, 100, ans + 544, good.size - 16, good.size - 1):
            o = Outputs(ft, [2 * BLK])
            status = torch.full((1,), 7, dtype=torch.uint8, device=DEV)
            call_range(dg, route, ft, 10, [garch[:cut].clone()], o.outs, [1], [2], status, torch.zeros((1,), dtype=torch.int32, device=DEV))
            assert status.item() == 0, (route, cut)
            o.check(0, 0, None)


@pytest.mark.parametrize("ft", [0, O.BFLOAT16])
def test_ranged_call_captured_in_a_hip_graph(dg, ft):
    sizes = [BLK * 33 + 1234, BLK * 17, BLK * 9]
    xs = [to_tensor(ft, make_words(ft, n, 40 + i)) for i, n in enumerate(sizes)]
    archs = gpu_archives(dg, ft, xs, 10)
    ranges = [(15, 4), (3, U32_MAX), (8, 1)]
    wants = [expected(t, f, c)[1] for t, (f, c) in zip(sizes, ranges)]
    outs = [torch.zeros((w,), dtype=FT_DTYPE[ft], device=DEV) for w in wants]
    status = torch.zeros((3,), dtype=torch.uint8, device=DEV)
    osz = torch.zeros((3,), dtype=torch.int32, device=DEV)

    def call():
        dg.decompress_data_range(ft != 0, archs, outs, [r[0] for r in ranges], [r[1] for r in ranges], None, status, osz)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warm: the parameter block becomes resident
            call()
    torch.cuda.synchronize()
    direct = [o.clone() for o in outs]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        call()
    torch.cuda.synchronize()
    for _ in range(2):
        for o in outs:
            o.zero_()
        status.zero_()
        osz.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert status.tolist() == [1, 1, 1] and osz.tolist() == wants
        for o, d, x, (first, _), w in zip(outs, direct, xs, ranges, wants):
            assert torch.equal(as_words(ft, o), as_words(ft, d))
            assert torch.equal(as_words(ft, o), as_words(ft, x)[first * BLK : first * BLK + w])
    del graph
    dg.lib().dgpu_release_graph_state()


@pytest.mark.parametrize("torch_ops", [True, False])
@pytest.mark.parametrize("ft", TYPES)
def test_slices_and_shards(dg, ft, torch_ops):
    from dietgpu_amd import distributed

    sizes = [BLK * 33 + 1234, BLK * 5, 1234, BLK * 8 + 1, 7]
    xs = [to_tensor(ft, make_words(ft, n, 60 + i)) for i, n in enumerate(sizes)]
    archs = gpu_archives(dg, ft, xs, 10)
    dg.prefer_torch_ops(torch_ops)
    try:
        for starts, counts in [([0, 0, 0, 0, 0], sizes), ([5000, 4096, 1233, 4095, 3], [70000, 8192, 1, 2, 0]),
                               ([BLK * 33 + 1233, BLK * 5, 0, BLK * 8, 7], [1, 0, 1, 1, 0])]:
            got = dg.decompress_data_slice(ft != 0, archs, starts, counts, dtype=FT_DTYPE[ft] if ft else None)
            for g, x, s0, c0 in zip(got, xs, starts, counts):
                assert g.dtype == x.dtype and g.numel() == c0
                assert torch.equal(as_words(ft, g), as_words(ft, x)[s0 : s0 + c0])
        with pytest.raises(RuntimeError):  # past the end of element 2
            dg.decompress_data_slice(ft != 0, archs, [0, 0, 1000, 0, 0], [1, 1, 235, 1, 1])
        if ft:
            with pytest.raises(RuntimeError):  # the archives hold another float type
                dg.decompress_data_slice(True, archs, [0] * 5, [1] * 5, dtype=torch.float32 if ft != O.FLOAT32 else torch.float16)
        world = 4
        shards = [distributed.decompress_shard(ft != 0, archs, r, world) for r in range(world)]  # every rank, one process
        for i, x in enumerate(xs):
            for r in range(world):
                lo, hi = distributed.shard_range(sizes[i], r, world)
                assert shards[r][i].numel() == hi - lo
            assert torch.equal(as_words(ft, torch.cat([shards[r][i] for r in range(world)])), as_words(ft, x))
        got = dg.decompress_data_slice(ft != 0, archs[:1], [12345], [23456], prob_bits=10)  # dtype from the header
        assert got[0].dtype == xs[0].dtype and torch.equal(as_words(ft, got[0]), as_words(ft, xs[0])[12345 : 12345 + 23456])
    finally:
        dg.prefer_torch_ops(True)
