"""dgpu_float_stochastic_compress on the GPU: float32 in, ordinary bfloat16 / float16 archives out, every rounding
stochastic.  Every archive is compared BYTE FOR BYTE with the reference of tests/stochastic_ref.py: the CPU oracle's
float_compress of the words sr_ref.sround gives with the random bits sr_ref.r16(seed, member, word index).  The histogram
pass and the encoder round every word in different kernels; a word on which they disagree reaches the encoder without a
probability and the archive differs (or the element fails), so the comparison covers the agreement of the two."""
import ctypes

import numpy as np
import pytest
import torch

import sr_ref as S
import stochastic_ref as SR

pytestmark = pytest.mark.gpu

BLK = 4096
FTS = [S.BFLOAT16, S.FLOAT16]
_TORCH = {S.BFLOAT16: torch.bfloat16, S.FLOAT16: torch.float16}
SIZES = [1, 7, 8, 9, 255, 256, 257, 4095, 4096, 4097, 2 * BLK + 5, 4 * BLK - 1, 4 * BLK + 300, 8 * BLK + 1, 17 * BLK + 250]
OFFSETS = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 0, 1, 2, 3, 1]  # float32 words past a 16-byte boundary, member by member
SEED64 = 0xFEDCBA9876543210


def _dev():
    return torch.device("cuda:0")


def _normal_bits(n, seed):
    """N(0, 1) * 2^k with k changing every few thousand words: compressible exponents over a wide range"""
    rng = np.random.default_rng(seed)
    k = rng.integers(-30, 30, n // 3000 + 1).repeat(3000)[:n]
    return (rng.standard_normal(n) * np.exp2(k)).astype(np.float32).view(np.uint32)


def _random_bits(n, seed):
    """any 32 bits: NaNs, infinities, denormals, and incompressible exponent bytes (the spill path)"""
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _upload(bits, offset_words=0):
    """float32 CUDA tensor of these bits, `offset_words` float32 words past a 16-byte boundary"""
    buf = torch.empty((bits.size + 8,), dtype=torch.float32, device=_dev())
    assert buf.data_ptr() % 16 == 0
    t = buf[offset_words : offset_words + bits.size]
    t.view(torch.int32).copy_(torch.from_numpy(bits.view(np.int32).copy()))
    return t


def _seed_tensor(seed):
    return torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.int64, device=_dev())


class Batch:
    """float32 elements (host bits) and, per (float type, probBits, seed, first member), what their archives must be"""

    def __init__(self, bits_list, offsets=None, tensors=None):
        self.bits = [np.ascontiguousarray(b, dtype=np.uint32) for b in bits_list]
        self.offsets = offsets or [0] * len(self.bits)
        self.tensors = tensors if tensors is not None else [_upload(b, o) for b, o in zip(self.bits, self.offsets)]
        self._want = {}

    def want(self, ft, prob_bits=10, seed=0, first=0):
        """-> (reference archives, their words)"""
        key = (ft, prob_bits, seed, first)
        if key not in self._want:
            pairs = [SR.archive(b, ft, seed, first + i, prob_bits) for i, b in enumerate(self.bits)]
            self._want[key] = ([a for a, _ in pairs], [w for _, w in pairs])
        return self._want[key]

    def same(self, comp, sizes, what, ft, prob_bits=10, seed=0, first=0, members=None):
        arch, _ = self.want(ft, prob_bits, seed, first)
        members = list(range(len(self.bits))) if members is None else members
        got_sizes, got = sizes.tolist(), comp.cpu().numpy()
        what = f"ft={ft} probBits={prob_bits} seed={seed:#x} first={first} {what}"
        assert got_sizes[: len(members)] == [int(arch[m].size) for m in members], what
        for row, m in enumerate(members):
            a = arch[m]
            bad = np.nonzero(got[row, : a.size] != a)[0]
            assert bad.size == 0, f"{what}: member {m} ({self.bits[m].size} words): {bad.size} bytes differ, the first at {bad[:4].tolist()}"

    def unchanged(self):
        for t, b in zip(self.tensors, self.bits):
            assert np.array_equal(t.view(torch.int32).cpu().numpy().view(np.uint32), b), "the input was modified"

    def run(self, what, ft, prob_bits=10, seed=0, first=0, members=None, seed_tensor=None):
        """one call through dietgpu_amd.ops, checked against the reference; `members`: a slice of the batch, called with
        the first member's number so that it draws the bits of the whole batch"""
        import dietgpu_amd as dg

        members = list(range(len(self.bits))) if members is None else members
        assert members == list(range(members[0], members[0] + len(members)))
        comp, sizes = dg.compress_data_stochastic([self.tensors[m] for m in members], _TORCH[ft], seed if seed_tensor is None else seed_tensor,
                                                  (first + members[0]) & 0xFFFFFFFF, prob_bits=prob_bits)
        self.same(comp, sizes, what, ft, prob_bits, seed, first, members)
        return comp, sizes


_cache = {}


def _cached(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def _mixed():
    """the sizes of tests/test_gpu_cast.py, N(0, 1) * 2^k and random bit patterns by turns, the sources at word offsets 0 to
    3 past a 16-byte boundary: at offsets 1 and 3 the histogram's 16-byte loads begin at an ODD index of the element"""
    return _cached("mixed", lambda: Batch([(_normal_bits if i % 3 else _random_bits)(n, 100 + i) for i, n in enumerate(SIZES)],
                                          offsets=OFFSETS))


def _cabi(batch, ft, prob_bits, seed, first, seed_dev=None):
    """the C ABI called directly -> (comp, sizes)"""
    import dietgpu_amd as dg

    L = dg.lib()
    B = len(batch.tensors)
    cap = int(L.dgpu_float_max_compressed_size(ft, max(b.size for b in batch.bits)))
    comp = torch.zeros((B, cap), dtype=torch.uint8, device=_dev())
    sizes = torch.zeros((B,), dtype=torch.int32, device=_dev())
    rc = L.dgpu_float_stochastic_compress(
        ft, prob_bits, B, (ctypes.c_void_p * B)(*[t.data_ptr() for t in batch.tensors]), (ctypes.c_uint32 * B)(*[b.size for b in batch.bits]),
        seed, None if seed_dev is None else ctypes.c_void_p(seed_dev.data_ptr()), first,
        (ctypes.c_void_p * B)(*[comp.data_ptr() + i * cap for i in range(B)]), ctypes.c_void_p(sizes.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.dgpu_last_error().decode()
    torch.cuda.synchronize()
    return comp, sizes


# ---------------------------------------------------------------------------------------------- 1. sizes, types, seeds
def test_the_offsets_cover_every_word_offset_at_small_and_large_sizes():
    b = _mixed()
    assert sorted({t.data_ptr() % 16 for t in b.tensors}) == [0, 4, 8, 12]
    assert {o for o, x in zip(b.offsets, b.bits) if x.size > 2 * BLK} == {0, 1, 2, 3}


@pytest.mark.parametrize("first", [0, 65534])
@pytest.mark.parametrize("seed", [0, SEED64])
@pytest.mark.parametrize("prob_bits", [9, 10, 11])
@pytest.mark.parametrize("ft", FTS)
def test_mixed_batch_on_both_routes(ft, prob_bits, seed, first):
    import dietgpu_amd as dg

    b = _mixed()
    comp, sizes = _cabi(b, ft, prob_bits, seed, first)
    b.same(comp, sizes, "C ABI", ft, prob_bits, seed, first)
    for torch_ops in (True, False):
        dg.prefer_torch_ops(torch_ops)
        try:
            b.run(f"torch_ops={torch_ops}", ft, prob_bits, seed, first)
        finally:
            dg.prefer_torch_ops(True)
    b.unchanged()


@pytest.mark.parametrize("ft", FTS)
def test_one_member_at_a_time_and_a_batch_split_in_two(ft):
    """every size alone (a call of its own geometry), and the batch as two calls: with first_member they draw the bits of
    the whole batch and give its bytes"""
    b = _mixed()
    for i in range(len(SIZES)):
        b.run(f"size {SIZES[i]} alone", ft, seed=SEED64, first=3, members=[i])
    b.run("members 0-5", ft, seed=SEED64, first=3, members=list(range(0, 6)))
    b.run("members 6-14", ft, seed=SEED64, first=3, members=list(range(6, len(SIZES))))
    # first_member + i is taken modulo 2^32
    b.run("wrapping member numbers", ft, seed=1, first=2**32 - 2, members=list(range(0, 6)))
    b.unchanged()


@pytest.mark.parametrize("ft", FTS)
def test_plain_compress_of_the_host_rounded_words_and_the_round_trip(ft):
    """the library's own dgpu_float_compress of the reference words gives the same archives, and every decoder reads them"""
    import dietgpu_amd as dg

    b = _mixed()
    comp, sizes = b.run("round trip", ft, seed=SEED64, first=9)
    _, words = b.want(ft, 10, SEED64, 9)
    t16 = [torch.from_numpy(w.view(np.int16).copy()).to(_dev()).view(_TORCH[ft]) for w in words]
    plain, psizes, _ = dg.compress_data(True, t16, False)
    assert psizes.tolist() == sizes.tolist()
    mask = torch.arange(comp.shape[1], device=_dev())[None, :] < sizes[:, None]
    assert plain.shape == comp.shape and torch.equal(torch.where(mask, plain, torch.zeros_like(plain)), torch.where(mask, comp, torch.zeros_like(comp)))
    rows = [comp[i, :n] for i, n in enumerate(sizes.tolist())]
    outs = [torch.empty((x.size,), dtype=_TORCH[ft], device=_dev()) for x in b.bits]
    status = torch.zeros((len(rows),), dtype=torch.uint8, device=_dev())
    dg.decompress_data(True, rows, outs, False, None, status, None)
    assert status.tolist() == [1] * len(rows)
    for i, w in enumerate(words):
        assert np.array_equal(outs[i].view(torch.int16).cpu().numpy().view(np.uint16), w), f"member {i}: decoded words"
    b.unchanged()


# --------------------------------------------------------------------------------------------------- 2. shapes and routes
@pytest.mark.parametrize("case,ft", [("rect", S.BFLOAT16), ("rect", S.FLOAT16), ("ragged", S.BFLOAT16), ("small-hw", S.BFLOAT16),
                                     ("small-hw", S.FLOAT16), ("deep", S.BFLOAT16), ("large", S.BFLOAT16), ("large", S.FLOAT16)])
def test_the_shapes_of_the_call_state_cases(case, ft):
    """rectangle, listed tiles, hardware dispatch with the spill pool, the two-level look-back over 65 tiles, and the
    histogram that 512 workgroups accumulate by atomics in the stream's counters"""
    import state_cases as C

    b = _cached(("case", case), lambda: Batch(C.case_bits32(case)))
    with C.hooks(C.CASES[case][2]):
        b.run(case, ft, seed=SEED64, first=1)
    b.unchanged()


def test_the_large_element_at_an_odd_word_offset():
    """the accumulate-by-atomics histogram with every vector load starting at an odd index of the element"""
    import state_cases as C

    bits = C.case_bits32("large")[0]
    b = Batch([bits], offsets=[3])
    b.run("large, 12 bytes past a boundary", S.BFLOAT16, seed=5)


@pytest.mark.parametrize("ft", FTS)
def test_thirty_members_in_three_size_classes(ft):
    import dietgpu_amd as dg

    sizes = [300, 2 * BLK + 100, 4 * BLK + 9] * 10
    b = _cached("classes30", lambda: Batch([(_normal_bits if i % 5 else _random_bits)(n + i % 7, 500 + i) for i, n in enumerate(sizes)],
                                           offsets=[i % 4 for i in range(len(sizes))]))
    L = dg.lib()
    try:
        for classes in (-1, 0, 1):
            for lists in (0, 1):
                L.dgpu_debug_set_size_classes(classes)
                L.dgpu_debug_set_work_lists(lists)
                b.run(f"size classes {classes} work lists {lists}", ft, seed=2, first=65534)
    finally:
        L.dgpu_debug_set_size_classes(-1)
        L.dgpu_debug_set_work_lists(-1)
    b.unchanged()


@pytest.mark.parametrize("ft", FTS)
def test_absent_workgroups_and_both_dispatch_modes(ft):
    import dietgpu_amd as dg

    L = dg.lib()
    b = _mixed()
    try:
        for absent in (0, 3):
            L.dgpu_debug_set_absent_workgroups(absent)
            for dispatch in (0, 1):
                L.dgpu_debug_set_encoder_dispatch(dispatch)
                b.run(f"absent workgroups {absent}, dispatch {dispatch}", ft, seed=SEED64, first=0)
    finally:
        L.dgpu_debug_set_absent_workgroups(0)
        L.dgpu_debug_set_encoder_dispatch(-1)


# ------------------------------------------------------------------------------------------------------------ 3. the seed
@pytest.mark.parametrize("ft", FTS)
def test_a_device_seed_gives_the_bytes_of_the_host_seed(ft):
    import dietgpu_amd as dg

    b = _mixed()
    for seed in (0, 1, SEED64, 2**64 - 1):
        held = _seed_tensor(seed)
        comp, sizes = _cabi(b, ft, 10, 0xDEAD, 0, seed_dev=held)  # (the host seed is not looked at beside a device one)
        b.same(comp, sizes, "C ABI, seed_dev", ft, 10, seed, 0)
        for torch_ops in (True, False):
            dg.prefer_torch_ops(torch_ops)
            try:
                b.run(f"tensor seed, torch_ops={torch_ops}", ft, seed=seed, seed_tensor=held)
            finally:
                dg.prefer_torch_ops(True)
        assert int(held.item()) & (2**64 - 1) == seed, "the seed tensor was written"


def test_other_seeds_and_members_give_other_words():
    b = _mixed()
    a0, _ = b.want(S.BFLOAT16, 10, 0, 0)
    a1, _ = b.want(S.BFLOAT16, 10, SEED64, 0)
    assert any(x.size != y.size or not np.array_equal(x, y) for x, y in zip(a0, a1))


# ------------------------------------------------------------------------------------------------- 4. the stream's state
@pytest.mark.parametrize("ft", FTS)
def test_same_bytes_after_a_rolling_and_a_reduce_compress_call(ft):
    """a counting encoder and a reduce-compress call ran on the stream before: the slab and the counters they leave do not
    reach this call's archives, and the counters are at rest after it"""
    import dietgpu_amd as dg

    L = dg.lib()
    b = _mixed()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ts = [torch.from_numpy(_normal_bits(n, 40 + i).view(np.int32).copy()).to(_dev()).view(torch.float32) for i, n in enumerate((3 * BLK + 7, 9 * BLK))]
    counts = torch.zeros((len(ts), 256), dtype=torch.int32, device=_dev())
    dg.compress_data_rolling(ts, None, counts, _TORCH[ft])
    dg.compress_data_rolling(ts, counts, counts, _TORCH[ft])
    b.run("after rolling-compress", ft, seed=SEED64)
    assert int(L.dgpu_debug_counters_nonzero(stream)) == 0
    t16 = [t.to(_TORCH[ft]) for t in ts]
    comp, sizes, _ = dg.compress_data(True, t16)
    rows = [[comp[i, : int(sizes[i])], comp[i, : int(sizes[i])]] for i in range(len(ts))]
    accs = [torch.empty_like(t) for t in ts]
    status = torch.zeros((len(ts),), dtype=torch.uint8, device=_dev())
    dg.decompress_data_reduce_compress(rows, accs, False, None, status, None, dtype=_TORCH[ft])
    assert status.tolist() == [1] * len(ts)
    b.run("after reduce-compress", ft, seed=SEED64)
    assert int(L.dgpu_debug_counters_nonzero(stream)) == 0
    b.unchanged()


@pytest.mark.parametrize("ft", FTS)
def test_a_captured_call_follows_the_seed_word(ft):
    """captured after one identical warm call; the seed word advanced between two replays: the archives of two eager calls
    with those seeds"""
    import dietgpu_amd as dg

    # (tensors of its own per float type: the float type is not part of a call's resident pointer / size block, and a block
    # that another stream uploaded makes the parameter cache query that upload's event, which a capturing thread may not do)
    b = _cached(("graph", ft), lambda: Batch([_normal_bits(5 * BLK + 3, 60), _random_bits(2 * BLK + 1, 61), _normal_bits(300, 62)], offsets=[1, 0, 2]))
    seed = 2**63 - 1  # (the int64 add wraps into the sign bit: the seed is the 64 bits)
    held = _seed_tensor(seed)
    cap = int(dg.lib().dgpu_float_max_compressed_size(ft, max(x.size for x in b.bits)))
    comp = torch.zeros((len(b.bits), cap), dtype=torch.uint8, device=_dev())
    sizes = torch.zeros((len(b.bits),), dtype=torch.int32, device=_dev())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dg.compress_data_stochastic(b.tensors, _TORCH[ft], held, 4, comp, sizes)  # the warm call, identical to the captured one
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=s):
            dg.compress_data_stochastic(b.tensors, _TORCH[ft], held, 4, comp, sizes)
        torch.cuda.synchronize()
        for step in range(2):
            comp.zero_()
            sizes.zero_()
            graph.replay()
            torch.cuda.synchronize()
            b.same(comp, sizes, f"replay {step}", ft, 10, (seed + step) & (2**64 - 1), 4)
            held.add_(1)
            torch.cuda.synchronize()
    finally:
        del graph
        dg.lib().dgpu_release_graph_state()  # (what the captured call pinned, as the header asks once the graph is gone)
    b.unchanged()
