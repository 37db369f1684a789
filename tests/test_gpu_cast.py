"""dgpu_float_cast_compress on the GPU: float32 in, ordinary bfloat16 / float16 archives out.  Every archive is compared
BYTE FOR BYTE with two references: the CPU oracle's float_compress of the words tests/cast_ref.py rounds on the host, and
the library's own plain dgpu_float_compress of the same words uploaded as 16-bit.  (The oracle writes zero where the
reference format leaves bytes indeterminate, as the library does: nothing needs masking.)"""
import ctypes

import numpy as np
import pytest
import torch

import cast_ref as R

pytestmark = pytest.mark.gpu

BLK = 4096
FTS = [R.BFLOAT16, R.FLOAT16]
_TORCH = {R.BFLOAT16: torch.bfloat16, R.FLOAT16: torch.float16}
SIZES = [1, 7, 8, 9, 255, 256, 257, 4095, 4096, 4097, 2 * BLK + 5, 4 * BLK - 1, 4 * BLK + 300, 8 * BLK + 1, 17 * BLK + 250]


def _dev():
    return torch.device("cuda:0")


def _normal_bits(n, seed):
    """N(0, 1) * 2^k with k changing every few thousand words: compressible exponents over a wide range"""
    rng = np.random.default_rng(seed)
    k = rng.integers(-30, 30, n // 3000 + 1).repeat(3000)[:n]
    return (rng.standard_normal(n) * np.exp2(k)).astype(np.float32).view(np.uint32)


def _random_bits(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _upload(bits, offset_words=0):
    """float32 CUDA tensor of these bits, `offset_words` float32 words past a 16-byte boundary"""
    buf = torch.empty((bits.size + 8,), dtype=torch.float32, device=_dev())
    assert buf.data_ptr() % 16 == 0
    t = buf[offset_words : offset_words + bits.size]
    t.view(torch.int32).copy_(torch.from_numpy(bits.view(np.int32).copy()))
    return t


class Batch:
    """float32 elements (host bits) and, per (float type, probBits), what their archives must be"""

    def __init__(self, bits_list, offsets=None):
        self.bits = [np.ascontiguousarray(b, dtype=np.uint32) for b in bits_list]
        self.offsets = offsets or [0] * len(self.bits)
        self.tensors = [_upload(b, o) for b, o in zip(self.bits, self.offsets)]
        self._want = {}

    def words(self, ft):
        return [R.cast_ref(b, ft) for b in self.bits]

    def want(self, ft, prob_bits=10):
        """-> (oracle archives, the same as a zero-padded [B, cap] matrix on the GPU, the validity mask, sizes)"""
        import dietgpu_amd as dg
        import oracle as O

        key = (ft, prob_bits)
        if key not in self._want:
            arch = [O.float_compress(ft, w, prob_bits) for w in self.words(ft)]
            cap = int(dg.lib().dgpu_float_max_compressed_size(ft, max(b.size for b in self.bits)))
            m = np.zeros((len(arch), cap), dtype=np.uint8)
            for i, a in enumerate(arch):
                m[i, : a.size] = a
            sizes = [int(a.size) for a in arch]
            mask = torch.arange(cap, device=_dev())[None, :] < torch.tensor(sizes, device=_dev())[:, None]
            self._want[key] = (arch, torch.from_numpy(m).to(_dev()), mask, sizes)
            # the second reference: the library's plain compress of the rounded words agrees with the first
            t16 = [torch.from_numpy(w.view(np.int16).copy()).to(_dev()).view(_TORCH[ft]) for w in self.words(ft)]
            comp, csz, _ = dg.compress_data(True, t16, False, prob_bits=prob_bits)
            self.same(comp, csz, ft, prob_bits, "plain dgpu_float_compress of the rounded words")
        return self._want[key]

    def same(self, comp, sizes, ft, prob_bits, what):
        arch, want, mask, want_sizes = self.want(ft, prob_bits)
        what = f"ft={ft} probBits={prob_bits} {what}"
        assert sizes.tolist() == want_sizes, what
        assert comp.shape == want.shape, what
        if torch.equal(torch.where(mask, comp, torch.zeros_like(comp)), want):
            return
        got = comp.cpu().numpy()
        for i, a in enumerate(arch):
            bad = np.nonzero(got[i, : a.size] != a)[0]
            assert bad.size == 0, f"{what}: member {i} ({self.bits[i].size} words): {bad.size} bytes differ, the first at {bad[:4].tolist()}"

    def unchanged(self):
        for t, b in zip(self.tensors, self.bits):
            assert np.array_equal(t.view(torch.int32).cpu().numpy().view(np.uint32), b), "the input was modified"


def _cast(batch, ft, what, prob_bits=10, members=None):
    """one call through dietgpu_amd.ops, checked against both references"""
    import dietgpu_amd as dg

    sub = batch if members is None else _sub(batch, members)
    comp, sizes, _ = dg.compress_data_cast(sub.tensors, _TORCH[ft], prob_bits=prob_bits)
    sub.same(comp, sizes, ft, prob_bits, what)
    return comp, sizes


_subs = {}


def _sub(batch, members):
    key = (id(batch), tuple(members))
    if key not in _subs:
        s = Batch.__new__(Batch)
        s.bits = [batch.bits[i] for i in members]
        s.offsets = [batch.offsets[i] for i in members]
        s.tensors = [batch.tensors[i] for i in members]
        s._want = {}
        _subs[key] = (s, batch)  # (keeps `batch` alive: the key is its id)
    return _subs[key][0]


_cache = {}


def _cached(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def _mixed():
    """the sizes of the issue, N(0, 1) * 2^k and random bit patterns by turns, sources at every word offset"""
    return _cached("mixed", lambda: Batch([(_normal_bits if i % 3 else _random_bits)(n, 100 + i) for i, n in enumerate(SIZES)],
                                          offsets=[i % 4 for i in range(len(SIZES))]))


def _classes300():
    """300 members of 3 size classes (2-, 4- and 8-block tiles; the single-block members run on the 2-block tiles)"""
    sizes = [300, 2 * BLK + 100, 4 * BLK + 9] * 100
    return _cached("classes300", lambda: Batch([(_normal_bits if i % 5 else _random_bits)(n + i % 7, 500 + i) for i, n in enumerate(sizes)]))


# --------------------------------------------------------------------------------------------------- 1. the conversion
@pytest.mark.parametrize("ft", FTS)
def test_edge_table_on_the_vector_path(ft):
    """every edge of the conversion in an element of several blocks: full-block chunks, and the table again in the last,
    partial block"""
    bits = np.concatenate([np.resize(R.EDGE_BITS, 2 * BLK), _normal_bits(BLK, 1), R.EDGE_BITS, R.EDGE_BITS[:37]])
    b = Batch([bits])
    _cast(b, ft, "edge table, vector path")
    b.unchanged()


@pytest.mark.parametrize("ft", FTS)
def test_edge_table_in_the_last_slice_and_on_the_scalar_path(ft):
    """the same values three at a time: as the last, partial 16-byte slice of a 43-word element (at a 16-byte boundary:
    aligned windows; 4 bytes past one: the load that ends at the element's last byte) and as an element below 16 bytes
    (at a boundary: tail form; past one: the scalar path)"""
    elems, offs = [], []
    for i in range(0, R.EDGE_BITS.size, 3):
        e = np.resize(R.EDGE_BITS[i : i + 3], 3)
        for off in (0, 1):
            elems += [np.concatenate([_normal_bits(40, i), e]), e]
            offs += [off, off]
    b = Batch(elems, offs)
    _cast(b, ft, "edge table, last slice and scalar path")
    b.unchanged()


@pytest.mark.parametrize("ft", FTS)
def test_every_word_carries_into_the_next_exponent(ft):
    """0x3fffffff rounds to 0x4000 in both types: a histogram of the unrounded exponent has no entry for the symbol"""
    b = Batch([np.full(2 * BLK + 17, 0x3FFFFFFF, dtype=np.uint32), np.full(5, 0x3FFFFFFF, dtype=np.uint32),
               np.full(9 * BLK + 3, 0xBFFFFFFF, dtype=np.uint32)], [0, 1, 3])
    assert (b.words(ft)[0] == 0x4000).all()
    for members in ([0], [1], [2], [0, 1, 2]):
        _cast(b, ft, f"carry elements {members}", members=members)


@pytest.mark.parametrize("ft", FTS)
def test_random_bit_patterns_and_scaled_normals(ft):
    """1 Mi uniformly random 32-bit patterns -- every exponent, NaN, inf; incompressible exponent bytes: the spill path
    and the pool hand-out -- and N(0, 1) * 2^k as the compressible case"""
    b = _cached("random", lambda: Batch([_random_bits(1 << 20, 7), _normal_bits(300000, 8), _random_bits(3 * BLK + 11, 9),
                                         _random_bits(BLK + 1, 10)]))
    for members in ([0], [1], [2, 3], [0, 1, 2, 3]):
        _cast(b, ft, f"random / normal elements {members}", members=members)
    b.unchanged()


# ------------------------------------------------------------------------------------------------------------ 2. sizes
@pytest.mark.parametrize("ft", FTS)
def test_sizes_one_member_at_a_time_and_as_one_batch(ft):
    b = _mixed()
    for i in range(len(SIZES)):
        _cast(b, ft, f"size {SIZES[i]} alone", members=[i])
    _cast(b, ft, "mixed batch")
    b.unchanged()


@pytest.mark.parametrize("ft", FTS)
def test_look_back_over_65_eight_block_tiles(ft):
    b = _cached("lookback", lambda: Batch([_normal_bits(65 * 8 * BLK, 11)]))
    _cast(b, ft, "65 tiles")


# ------------------------------------------------------------------------------------------------------ 3. host routes
@pytest.mark.parametrize("which", ["mixed", "classes300"])
@pytest.mark.parametrize("ft", FTS)
def test_forced_host_routes(ft, which):
    """both encoder dispatch forms, work lists on and off, size classes on, off and under the policy, parameter cache
    on and off: the archives do not depend on the route"""
    import dietgpu_amd as dg

    L = dg.lib()
    b = _mixed() if which == "mixed" else _classes300()
    b.want(ft)
    try:
        for dispatch in (0, 1):
            for lists in (0, 1):
                for classes in (-1, 0, 1):
                    for cache in (1, 0):
                        L.dgpu_debug_set_encoder_dispatch(dispatch)
                        L.dgpu_debug_set_work_lists(lists)
                        L.dgpu_debug_set_size_classes(classes)
                        L.dgpu_debug_set_param_cache(cache)
                        _cast(b, ft, f"{which}: dispatch {dispatch} work lists {lists} size classes {classes} parameter cache {cache}")
    finally:
        L.dgpu_debug_set_encoder_dispatch(-1)
        L.dgpu_debug_set_work_lists(-1)
        L.dgpu_debug_set_size_classes(-1)
        L.dgpu_debug_set_param_cache(1)
    b.unchanged()


# -------------------------------------------------------------------------------------------------------- 4. alignment
@pytest.mark.parametrize("ft", FTS)
def test_sources_at_every_word_offset(ft):
    sizes = [3, 43, BLK + 300, 8 * BLK + 1]
    b = Batch([_normal_bits(n, 20 + off) for off in range(4) for n in sizes], [off for off in range(4) for _ in sizes])
    assert sorted({t.data_ptr() % 16 for t in b.tensors}) == [0, 4, 8, 12]
    for i in range(len(b.bits)):
        _cast(b, ft, f"{b.bits[i].size} words at byte offset {4 * b.offsets[i]}", members=[i])
    _cast(b, ft, "all offsets in one batch")


@pytest.mark.parametrize("ft", FTS)
def test_rows_of_one_matrix_and_a_scrambled_pointer_list(ft):
    """rows of an odd width: an arithmetic progression of 4-byte aligned addresses (stride views), then the same rows in
    a scrambled order (an uploaded pointer list)"""
    import dietgpu_amd as dg

    rows, width = 12, 2 * BLK + 301
    bits = _normal_bits(rows * width, 30).reshape(rows, width)
    m = torch.from_numpy(bits.view(np.int32).copy()).to(_dev()).view(torch.float32)
    for order in (list(range(rows)), [7, 2, 11, 0, 5, 9, 1, 10, 3, 8, 6, 4]):
        b = Batch.__new__(Batch)
        b.bits, b.offsets, b.tensors, b._want = [bits[i] for i in order], [0] * rows, [m[i] for i in order], {}
        comp, sizes, _ = dg.compress_data_cast(b.tensors, _TORCH[ft])
        b.same(comp, sizes, ft, 10, f"matrix rows in order {order}")


# ----------------------------------------------------------------------------------------------- 5. precision and routes
def _cabi(batch, ft, prob_bits):
    """the C ABI called directly, with the temp region its contract names -> (comp, sizes, tempUsed, contract)"""
    import dietgpu_amd as dg

    L = dg.lib()
    B = len(batch.tensors)
    mx = max(b.size for b in batch.bits)
    cap = int(L.dgpu_float_max_compressed_size(ft, mx))
    contract = int(L.dgpu_float_compress_temp_bytes(ft, B, mx))
    temp = torch.empty((contract,), dtype=torch.uint8, device=_dev())
    comp = torch.zeros((B, cap), dtype=torch.uint8, device=_dev())
    sizes = torch.zeros((B,), dtype=torch.int32, device=_dev())
    used = ctypes.c_size_t(0)
    rc = L.dgpu_float_cast_compress(
        ctypes.c_void_p(temp.data_ptr()), contract, ctypes.byref(used), ft, prob_bits, B,
        (ctypes.c_void_p * B)(*[t.data_ptr() for t in batch.tensors]), (ctypes.c_uint32 * B)(*[b.size for b in batch.bits]),
        (ctypes.c_void_p * B)(*[comp.data_ptr() + i * cap for i in range(B)]), ctypes.c_void_p(sizes.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.dgpu_last_error().decode()
    torch.cuda.synchronize()
    return comp, sizes, int(used.value), contract


@pytest.mark.parametrize("prob_bits", [9, 10, 11])
@pytest.mark.parametrize("ft", FTS)
def test_prob_bits_on_the_c_abi_and_the_temp_contract(ft, prob_bits):
    b = _mixed()
    comp, sizes, used, contract = _cabi(b, ft, prob_bits)
    b.same(comp, sizes, ft, prob_bits, "C ABI, mixed batch")
    assert 0 < used <= contract, (used, contract)  # dgpu_float_compress_temp_bytes of the ARCHIVE's type is the contract
    for members in ([0], [3], [14]):  # the smallest, a single-block and the largest member alone
        s = _sub(b, members)
        comp, sizes, used, contract = _cabi(s, ft, prob_bits)
        s.same(comp, sizes, ft, prob_bits, f"C ABI, member {members}")
        assert used <= contract, (used, contract)


@pytest.mark.parametrize("torch_ops", [True, False])
@pytest.mark.parametrize("ft", FTS)
def test_op_route_and_ctypes_route(ft, torch_ops):
    import dietgpu_amd as dg

    b = _mixed()
    dg.prefer_torch_ops(torch_ops)
    try:
        _cast(b, ft, f"torch_ops={torch_ops}")
        # caller's output tensors and temp memory, as compress_data takes them
        _, want, _, _ = b.want(ft)
        out = torch.zeros((len(b.bits) + 1, want.shape[1] + 16), dtype=torch.uint8, device=_dev())
        osz = torch.zeros((len(b.bits) + 1,), dtype=torch.int32, device=_dev())
        temp = torch.empty((int(dg.lib().dgpu_float_compress_temp_bytes(ft, len(b.bits), max(SIZES))),), dtype=torch.uint8, device=_dev())
        comp, sizes, used = dg.compress_data_cast(b.tensors, _TORCH[ft], temp, out, osz)
        assert comp.data_ptr() == out.data_ptr() and sizes.data_ptr() == osz.data_ptr() and 0 < used <= temp.numel()
        b.same(comp[: len(b.bits), : want.shape[1]].contiguous(), sizes[: len(b.bits)], ft, 10, f"torch_ops={torch_ops}, caller's outputs")
    finally:
        dg.prefer_torch_ops(True)


# ----------------------------------------------------------------------------------------------------- 6. round trip
@pytest.mark.parametrize("ft", FTS)
def test_round_trip_through_the_existing_decoders(ft):
    import dietgpu_amd as dg

    b = _mixed()
    comp, sizes = _cast(b, ft, "round trip")
    rows = [comp[i, :n] for i, n in enumerate(sizes.tolist())]
    outs = [torch.empty((x.size,), dtype=_TORCH[ft], device=_dev()) for x in b.bits]
    status = torch.zeros((len(rows),), dtype=torch.uint8, device=_dev())
    dg.decompress_data(True, rows, outs, False, None, status, None)
    wide = [torch.full((x.size,), 7.0, dtype=torch.float32, device=_dev()) for x in b.bits]
    status2 = torch.zeros((len(rows),), dtype=torch.uint8, device=_dev())
    dg.decompress_data_accumulate(rows, wide, False, None, status2, None, dtype=_TORCH[ft])
    assert status.tolist() == [1] * len(rows) and status2.tolist() == [1] * len(rows)
    for i, w in enumerate(b.words(ft)):
        assert np.array_equal(outs[i].view(torch.int16).cpu().numpy().view(np.uint16), w), f"member {i}: decoded words"
        assert np.array_equal(wide[i].view(torch.int32).cpu().numpy().view(np.uint32), R.widen(w, ft)), f"member {i}: widened words"
    b.unchanged()
