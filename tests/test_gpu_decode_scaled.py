"""Scaled decompress on the GPU (dgpu_float_decode_scaled, k_ans_decode_scaled): float archives decoded with every
word multiplied by a float32 factor -- a host float, one device float, or one device float per member -- and rounded
once to the type.  The inputs are oracle archives of the cases of tests/accum_cases.py (premises:
tests/test_decode_scaled_host.py); every expected word comes from tests/scaled_ref.py and is compared BIT FOR BIT on
integer views."""
import ctypes

import numpy as np
import pytest
import torch

import accum_cases as C
import scaled_ref as S
from test_decode_scaled_host import FACTORS, THIRD
from test_gpu_accumulate import _dev
from test_gpu_accumulate_paths import _rows, _same

pytestmark = pytest.mark.gpu

GUARD = 64
MODES = ("host", "dev1", "devn")
_want_cache = {}


def _storage(ft):
    return torch.int32 if ft == S.FLOAT32 else torch.int16


def _pattern(ft, byte):
    """a word of the type's width with every byte `byte`, as the signed integer torch fills with"""
    v = int.from_bytes(bytes([byte]) * (4 if ft == S.FLOAT32 else 2), "little", signed=True)
    return v


class Out:
    """An output of n words of float type ft, `offset` words past a 16-byte boundary, 64 guard words on each side."""

    def __init__(self, ft, n, offset=0, fill=0xCD):
        self.ft, self.n, self.lo = ft, n, GUARD + offset
        self.sentinel = _pattern(ft, 0xCD)
        self.buf = torch.full((self.lo + n + GUARD,), self.sentinel, dtype=_storage(ft), device=_dev())
        if fill != 0xCD:
            self.buf[self.lo : self.lo + n].fill_(_pattern(ft, fill))
        self.view = self.buf[self.lo : self.lo + n].view(C.DTYPE[ft])

    def bits(self):
        return self.buf[self.lo : self.lo + self.n].cpu().numpy().view(C.WORD[self.ft])

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[: self.lo] == self.sentinel).all() and (b[self.lo + self.n :] == self.sentinel).all())


def _want(case, i, factor):
    key = (case.tag, case.ft, i, float(factor))
    if key not in _want_cache:
        _want_cache[key] = S.scaled_ref(case.words[i], case.ft, factor)
    return _want_cache[key]


def _factors_of(mode, B, k0=0):
    """-> (the `scale` argument, the factor of every member)"""
    if mode == "devn":
        fs = [FACTORS[(k0 + k) % len(FACTORS)] for k in range(B)]
        return torch.tensor([float(f) for f in fs], dtype=torch.float32, device=_dev()), fs
    f = FACTORS[k0 % len(FACTORS)]
    if mode == "dev1":
        return torch.tensor([float(f)], dtype=torch.float32, device=_dev()), [f] * B
    return float(f), [f] * B


def _decode_batch(case, prob_bits, members, mode, k0, what, offsets=None):
    """one call for `members` of the case: status, sizes, every word and the guards"""
    import dietgpu_amd as dg

    rows = _rows(case, prob_bits)
    B = len(members)
    scale, fs = _factors_of(mode, B, k0)
    outs = [Out(case.ft, case.sizes[i], offsets[k] if offsets else 0) for k, i in enumerate(members)]
    status = torch.full((B,), 7, dtype=torch.uint8, device=_dev())
    sizes = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    used = dg.decompress_data_scaled([rows[i] for i in members], [o.view for o in outs], scale, None, status, sizes, prob_bits=prob_bits)
    what = f"{case.tag} ft={case.ft} probBits={prob_bits} {mode} factors from {k0}: {what}"
    assert used == 0, what
    assert status.tolist() == [1] * B, what
    assert sizes.tolist() == [case.sizes[i] for i in members], what
    for k, (i, o) in enumerate(zip(members, outs)):
        _same(o.bits(), _want(case, i, fs[k]), f"{what}: member {k} ({case.sizes[i]} words, factor {float(fs[k])!r})")
        assert o.guards_intact(), f"{what}: member {k} ({case.sizes[i]} words): guard words overwritten"


# ------------------------------------------------------------------------------------------------ 1. staging modes
@pytest.mark.parametrize("route", ["torch_ops", "ctypes"])
@pytest.mark.parametrize("prob_bits", C.PROB_BITS)
@pytest.mark.parametrize("ft", C.FTS)
def test_staging_modes(ft, prob_bits, route):
    """whole-staged, ring, mixed and boundary waves, 16-block and 4-block tiles, every way to pass the factor and every
    factor: each element alone, then all together"""
    import dietgpu_amd as dg

    case = C.staging(ft, 0)
    everything = list(range(len(case.sizes)))
    dg.prefer_torch_ops(route == "torch_ops")
    try:
        for n, members in enumerate([[i] for i in everything] + [everything]):
            for m, mode in enumerate(MODES):
                _decode_batch(case, prob_bits, members, mode, n + m, f"{route}, members {members}")
        for k0 in range(len(FACTORS)):  # every factor on every element, through the host float and the single device float
            for mode in ("host", "dev1"):
                _decode_batch(case, prob_bits, everything, mode, k0, f"{route}, all members")
    finally:
        dg.prefer_torch_ops(True)


# ---------------------------------------------------------------------------------------- 2. partial last blocks
@pytest.mark.parametrize("lead", C.LEADS)
@pytest.mark.parametrize("ft", C.FTS)
def test_partial_last_blocks_at_every_row_count(ft, lead):
    """last blocks of 1 .. 4095 words on both sides of the 8-row group boundaries, behind 0, 1, 3 or 8 whole blocks,
    outputs at every word offset from a 16-byte boundary"""
    case = C.tails(ft, lead)
    members = list(range(len(case.sizes)))
    per16 = 4 if ft == S.FLOAT32 else 8
    for m, mode in enumerate(MODES):
        _decode_batch(case, 10, members, mode, lead + m, f"lead {lead}", offsets=[i % per16 for i in members])
    _decode_batch(case, 10, members, "devn", lead + 2, f"lead {lead}, shifted factors", offsets=[(i + 3) % per16 for i in members])


# ------------------------------------------------------------------------------------------- 3. workgroup orders
@pytest.mark.parametrize("B", C.ORDER_BATCHES)
@pytest.mark.parametrize("ft", C.FTS)
def test_workgroup_orders(ft, B):
    """element-major, tile-major and per-XCD order in both tile geometries, then the work list forced on and off"""
    import dietgpu_amd as dg

    L = dg.lib()
    for tile_blocks in C.ORDER_GEOMETRIES:
        case = C.orders(ft, B, tile_blocks)
        members = list(range(B))
        assert -(-max(case.sizes) // C.BLK) == C.ORDER_GEOMETRIES[tile_blocks][1]  # this geometry
        for order in (-1, 0, 1, 2):
            L.dgpu_debug_set_decoder_order(order)
            try:
                _decode_batch(case, 10, members, "devn", 0, f"order {order}, {tile_blocks}-block tiles")
            finally:
                L.dgpu_debug_set_decoder_order(-1)
        if B == min(C.ORDER_BATCHES):
            _decode_batch(case, 10, members, "host", 0, f"{tile_blocks}-block tiles")
            _decode_batch(case, 10, members, "dev1", 1, f"{tile_blocks}-block tiles")
        if B == max(C.ORDER_BATCHES):
            for lists in (1, 0):
                L.dgpu_debug_set_work_lists(lists)
                try:
                    _decode_batch(case, 10, members, "devn", 0, f"work lists {lists}, {tile_blocks}-block tiles")
                finally:
                    L.dgpu_debug_set_work_lists(-1)


# ------------------------------------------------------------------------------ 4. capacity larger than the element
@pytest.mark.parametrize("ft", C.FTS)
def test_capacity_larger_than_the_element(ft):
    """the geometry comes from the capacity: tiles and half-waves past the element's end run, and must leave the words
    [size, capacity) of the output alone"""
    import dietgpu_amd as dg

    case = C.capacity(ft)
    rows = _rows(case, 10)
    rules = list(C.CAPACITY_RULES.items())
    everything = list(range(len(case.sizes)))
    batches = [([i], [rule(case.sizes[i])], f"element {i} alone, capacity {name}") for i in everything for name, rule in rules]
    batches += [(everything, [rule(n) for n in case.sizes], f"all, capacity {name}") for name, rule in rules]
    batches += [(everything, [rules[(i + 1) % len(rules)][1](n) for i, n in enumerate(case.sizes)], "all, assorted capacities")]
    planted = np.array([_pattern(ft, 0xA5)], dtype=np.int64).astype(C.SIGNED[ft]).view(C.WORD[ft])[0]
    for b, (members, caps, what) in enumerate(batches):
        mode = MODES[b % 3]
        scale, fs = _factors_of(mode, len(members), b)
        outs = [Out(ft, cap, fill=0xA5) for cap in caps]
        status = torch.full((len(members),), 7, dtype=torch.uint8, device=_dev())
        sizes = torch.full((len(members),), -7, dtype=torch.int32, device=_dev())
        dg.decompress_data_scaled([rows[i] for i in members], [o.view for o in outs], scale, None, status, sizes)
        what2 = f"ft={ft} {mode} {what}"
        assert status.tolist() == [1] * len(members), what2
        assert sizes.tolist() == [case.sizes[i] for i in members], what2
        for k, (i, o) in enumerate(zip(members, outs)):
            got, n = o.bits(), case.sizes[i]
            _same(got[:n], _want(case, i, fs[k]), f"{what2}: element {i}")
            assert (got[n:] == planted).all(), f"{what2}: element {i}: words past its size were written"
            assert o.guards_intact(), f"{what2}: element {i}: guard words overwritten"


# -------------------------------------------------------------------------------------- 5. malformed descriptors
@pytest.mark.parametrize("name", list(C.MALFORMED_BATCHES))
@pytest.mark.parametrize("ft", C.FTS)
def test_a_malformed_member_fails_alone(ft, name):
    """status 0 for the corrupted member; both neighbours are exact"""
    import dietgpu_amd as dg

    tile_blocks, sizes, cap1 = C.MALFORMED_BATCHES[name]
    case = C.malformed(ft, name)
    rows = _rows(case, 10)
    caps = [sizes[0], cap1, sizes[2]]
    for c, (what, bad) in enumerate(C.corruptions(ft, case.archives(10)[1], sizes[1], tile_blocks)):
        mode = MODES[c % 3]
        scale, fs = _factors_of(mode, 3, c)
        ins = [rows[0], torch.from_numpy(bad).to(_dev()), rows[2]]
        outs = [Out(ft, cap) for cap in caps]
        status = torch.full((3,), 7, dtype=torch.uint8, device=_dev())
        out_sizes = torch.full((3,), -7, dtype=torch.int32, device=_dev())
        dg.decompress_data_scaled(ins, [o.view for o in outs], scale, None, status, out_sizes)
        what2 = f"ft={ft} {name}, {what}, {mode}"
        assert status.tolist() == [1, 0, 1], what2
        assert out_sizes.tolist() == sizes, what2  # the header is valid in every case
        for k in (0, 2):
            _same(outs[k].bits(), _want(case, k, fs[k]), f"{what2}: neighbour {k}")
        assert all(o.guards_intact() for o in outs), what2 + ": guard words overwritten"


# ------------------------------------------------------------------------------------------- 6. particular factors
@pytest.mark.parametrize("ft", C.FTS)
def test_device_factor_one_is_the_plain_decode(ft):
    import dietgpu_amd as dg

    for case in (C.staging(ft, 1), C.tails(ft, 3)):
        rows = _rows(case, 10)
        plain = [Out(ft, n) for n in case.sizes]
        status = torch.zeros(len(rows), dtype=torch.uint8, device=_dev())
        dg.decompress_data(True, rows, [o.view for o in plain], False, None, status, None)
        assert status.tolist() == [1] * len(rows)
        for scale in (torch.ones(1, dtype=torch.float32, device=_dev()), torch.ones(len(rows), dtype=torch.float32, device=_dev())):
            outs = [Out(ft, n) for n in case.sizes]
            status.zero_()
            dg.decompress_data_scaled(rows, [o.view for o in outs], scale, None, status, None)
            assert status.tolist() == [1] * len(rows)
            for i, (o, p) in enumerate(zip(outs, plain)):
                _same(o.bits(), p.bits(), f"{case.tag} ft={ft} element {i}, a device factor of 1.0 against decompress_data")
                _same(o.bits(), case.words[i], f"{case.tag} ft={ft} element {i}, a device factor of 1.0 against the input")
        # a host factor whose float32 is 1.0 IS the plain call
        outs = [Out(ft, n) for n in case.sizes]
        dg.decompress_data_scaled(rows, [o.view for o in outs], 1.0 + 1e-12, None, status, None)
        for i, o in enumerate(outs):
            _same(o.bits(), case.words[i], f"{case.tag} ft={ft} element {i}, host factor 1.0")


def _special_words(ft, with_nonfinite):
    """a block and a bit of every kind of word: zeros, denormals, the largest and smallest normals, ordinary values --
    and, planted, +-inf and NaNs, one with a payload in the low bits only"""
    if ft == S.FLOAT32:
        pats = [0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x807FFFFF, 0x00400000, 0x00800000, 0x3F800000,
                0xBF800001, 0x40490FDB, 0x3EAAAAAB, 0x7F000000]
        extra = [0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001]
    elif ft == S.FLOAT16:
        pats = [0x0000, 0x8000, 0x7BFF, 0xFBFF, 0x0001, 0x83FF, 0x0200, 0x0400, 0x3C00, 0xBC01, 0x4248, 0x3555, 0x7800]
        extra = [0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7C01]
    else:
        pats = [0x0000, 0x8000, 0x7F7F, 0xFF7F, 0x0001, 0x807F, 0x0040, 0x0080, 0x3F80, 0xBF81, 0x4049, 0x3EAB, 0x7F00]
        extra = [0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F81]
    return np.resize(np.array(pats + (extra if with_nonfinite else []), dtype=C.WORD[ft]), C.BLK + 4097)


def _compress_words(ft, w):
    import dietgpu_amd as dg

    t = torch.from_numpy(w.view(C.SIGNED[ft]).copy()).view(C.DTYPE[ft]).to(_dev())
    comp, sizes, _ = dg.compress_data(True, [t], False, None)
    return comp[0, : int(sizes[0])]


def _check_against_reference(ft, w, row, scale, factor, what):
    import dietgpu_amd as dg

    want = S.scaled_ref(w, ft, factor)
    o = Out(ft, w.size)
    status = torch.zeros(1, dtype=torch.uint8, device=_dev())
    dg.decompress_data_scaled([row], [o.view], scale, None, status, None)
    assert status.tolist() == [1], what
    got = o.bits()
    nan = S.is_nan(want, ft)
    assert S.is_nan(got, ft)[nan].all(), f"{what}: a NaN of the reference is not a NaN"
    assert not S.is_inf(got, ft)[nan].any(), f"{what}: a NaN became an infinity"
    assert not S.is_nan(got, ft)[~nan].any(), f"{what}: a NaN where the reference has none"
    _same(got[~nan], want[~nan], what)
    assert o.guards_intact(), what
    return want, nan


@pytest.mark.parametrize("ft", C.FTS)
def test_device_factors_zero_and_infinity(ft):
    """finite words, zeros of both signs among them: 0.0 gives signed zeros, +inf gives infinities and NaN for the zeros"""
    w = _special_words(ft, False)
    row = _compress_words(ft, w)
    top = C.WORD[ft](1 << (31 if ft == S.FLOAT32 else 15))
    for factor in (0.0, -0.0, float("inf"), float("-inf")):
        scale = torch.tensor([factor], dtype=torch.float32, device=_dev())
        want, nan = _check_against_reference(ft, w, row, scale, factor, f"ft={ft} device factor {factor!r}")
        if factor == 0.0:
            assert not nan.any() and ((want & ~top) == 0).all() and (want != 0).any() and (want == 0).any()
        else:
            zero = (w & ~top) == 0
            assert np.array_equal(nan, zero) and S.is_inf(want, ft)[~zero].all()


@pytest.mark.parametrize("ft", C.FTS)
def test_planted_infinities_and_nans(ft):
    w = _special_words(ft, True)
    row = _compress_words(ft, w)
    for factor in (THIRD, np.float32(-1.5), np.float32(3.0e38), np.float32(2.0 ** -20), np.float32(1.0), np.float32(0.0)):
        scale = torch.tensor([float(factor)], dtype=torch.float32, device=_dev())
        _, nan = _check_against_reference(ft, w, row, scale, factor, f"ft={ft} device factor {float(factor)!r}")
        assert nan.any() and (~nan).any()
        if factor not in (np.float32(1.0), np.float32(0.0)):
            _check_against_reference(ft, w, row, float(factor), factor, f"ft={ft} host factor {float(factor)!r}")


def test_an_archive_of_another_float_type_gets_status_0():
    import dietgpu_amd as dg

    bf, fp = C.staging(S.BFLOAT16, 0), C.staging(S.FLOAT16, 0)
    rows = [_rows(bf, 10)[1], _rows(fp, 10)[1], _rows(bf, 10)[2]]
    n = [bf.sizes[1], fp.sizes[1], bf.sizes[2]]
    outs = [Out(S.BFLOAT16, k) for k in n]
    status = torch.full((3,), 7, dtype=torch.uint8, device=_dev())
    scale = torch.tensor([float(THIRD)], dtype=torch.float32, device=_dev())
    dg.decompress_data_scaled(rows, [o.view for o in outs], scale, None, status, None)
    assert status.tolist() == [1, 0, 1]
    _same(outs[0].bits(), _want(bf, 1, THIRD), "left neighbour")
    _same(outs[2].bits(), _want(bf, 2, THIRD), "right neighbour")
    assert all(o.guards_intact() for o in outs)


def test_bare_c_abi_with_a_stride_of_one():
    import dietgpu_amd as dg

    case = C.staging(S.BFLOAT16, 0)
    rows = _rows(case, 10)
    B = len(rows)
    fs = [FACTORS[k % len(FACTORS)] for k in range(B)]
    scale = torch.tensor([float(f) for f in fs], dtype=torch.float32, device=_dev())
    outs = [Out(S.BFLOAT16, n) for n in case.sizes]
    status = torch.zeros(B, dtype=torch.uint8, device=_dev())
    used = ctypes.c_size_t(99)
    rc = dg.lib().dgpu_float_decode_scaled(
        None, 0, ctypes.byref(used), S.BFLOAT16, 10, B, (ctypes.c_void_p * B)(*[r.data_ptr() for r in rows]),
        (ctypes.c_uint32 * B)(*[r.numel() for r in rows]), (ctypes.c_void_p * B)(*[o.view.data_ptr() for o in outs]),
        (ctypes.c_uint32 * B)(*case.sizes), 1.0, ctypes.c_void_p(scale.data_ptr()), 1, ctypes.c_void_p(status.data_ptr()), None,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and used.value == 0, dg.lib().dgpu_last_error()
    assert status.tolist() == [1] * B
    for i, o in enumerate(outs):
        _same(o.bits(), _want(case, i, fs[i]), f"element {i}")


# ---------------------------------------------------------------------------------------------------- 7. capture
def test_graph_replay_follows_the_factor_in_memory():
    """one linear capture of a call with a device factor (a host synchronisation inside the call would end the capture
    with an error); replayed after the factor tensor is overwritten, the output follows the NEW value"""
    import dietgpu_amd as dg

    ft = S.BFLOAT16
    case = C.staging(ft, 0)
    members = [0, 2]
    rows = [_rows(case, 10)[i] for i in members]
    outs = [Out(ft, case.sizes[i]) for i in members]
    views = [o.view for o in outs]
    status = torch.zeros(2, dtype=torch.uint8, device=_dev())
    scale = torch.tensor([float(THIRD)], dtype=torch.float32, device=_dev())

    def call():
        dg.decompress_data_scaled(rows, views, scale, None, status, None)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # makes the parameter block resident
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        call()
    torch.cuda.synchronize()
    try:
        for factor in (np.float32(-1.5), np.float32(2.0 ** -20), THIRD):
            scale.fill_(float(factor))
            for o in outs:
                o.buf[o.lo : o.lo + o.n].fill_(o.sentinel)
            status.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert status.tolist() == [1, 1]
            for k, i in enumerate(members):
                _same(outs[k].bits(), _want(case, i, factor), f"replay with {float(factor)!r} in the factor tensor, element {i}")
                assert outs[k].guards_intact()
    finally:
        del graph
        dg.lib().dgpu_release_graph_state()
