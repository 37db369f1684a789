"""Scaled decode-accumulate on the GPU (dgpu_float_decode_accumulate_scaled, k_ans_decode_accum_scaled): float archives
decoded into float32 accumulators as acc = [acc +] fl32(widen(word) * s), the factor a host float, one device float, or
one device float per member.  The inputs are oracle archives of the cases of tests/accum_cases.py (premise:
tests/test_accum_scaled_host.py); every expected word comes from tests/accum_scaled_ref.py and is compared BIT FOR BIT
on integer views.  Every accumulator has 64 guard words on each side."""
import ctypes

import numpy as np
import pytest
import torch

import accum_cases as C
import accum_scaled_ref as A
from test_decode_scaled_host import FACTORS, THIRD
from test_gpu_accumulate import Acc, _dev
from test_gpu_accumulate_paths import SENTINEL2, _rows, _same

pytestmark = pytest.mark.gpu

MODES = ("host", "dev1", "devn")
_want_cache = {}


def _want(case, i, factor, accumulate):
    key = (case.tag, case.ft, i, float(factor), bool(accumulate))
    if key not in _want_cache:
        _want_cache[key] = A.accum_scaled_ref(case.words[i], case.ft, factor, C.bits(case.start[i]) if accumulate else None)
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


def _decode_batch(case, prob_bits, members, mode, k0, accumulate, what, offsets=None):
    """one call for `members` of the case: status, sizes, every accumulator word and the guards"""
    import dietgpu_amd as dg

    rows = _rows(case, prob_bits)
    B = len(members)
    scale, fs = _factors_of(mode, B, k0)
    accs = [Acc(case.sizes[i], offsets[k] if offsets else 0, fill=case.start[i] if accumulate else None) for k, i in enumerate(members)]
    status = torch.full((B,), 7, dtype=torch.uint8, device=_dev())
    sizes = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    used = dg.decompress_data_accumulate([rows[i] for i in members], [a.view for a in accs], accumulate, None, status, sizes,
                                         prob_bits=prob_bits, dtype=C.DTYPE[case.ft], scale=scale)
    what = f"{case.tag} ft={case.ft} probBits={prob_bits} accumulate={accumulate} {mode} factors from {k0}: {what}"
    assert used == 0, what
    assert status.tolist() == [1] * B, what
    assert sizes.tolist() == [case.sizes[i] for i in members], what
    for k, (i, a) in enumerate(zip(members, accs)):
        _same(a.bits(), _want(case, i, fs[k], accumulate), f"{what}: member {k} ({case.sizes[i]} words, factor {float(fs[k])!r})")
        assert a.guards_intact(), f"{what}: member {k} ({case.sizes[i]} words): guard words overwritten"


# ------------------------------------------------------------------------------------------------ 1. staging modes
@pytest.mark.parametrize("route", ["torch_ops", "ctypes"])
@pytest.mark.parametrize("prob_bits", C.PROB_BITS)
@pytest.mark.parametrize("ft", C.FTS)
def test_staging_modes(ft, prob_bits, route):
    """whole-staged, ring, mixed and boundary waves, 16-block and 4-block tiles, every way to pass the factor, store and
    add: each element alone, then all together"""
    import dietgpu_amd as dg

    case = C.staging(ft, 0)
    everything = list(range(len(case.sizes)))
    dg.prefer_torch_ops(route == "torch_ops")
    try:
        for n, members in enumerate([[i] for i in everything] + [everything]):
            for m, mode in enumerate(MODES):
                for accumulate in (False, True):
                    _decode_batch(case, prob_bits, members, mode, n + m, accumulate, f"{route}, members {members}")
        for k0 in range(len(FACTORS)):  # every factor on every element
            _decode_batch(case, prob_bits, everything, "dev1", k0, True, f"{route}, all members")
    finally:
        dg.prefer_torch_ops(True)


# ---------------------------------------------------------------------------------------- 2. partial last blocks
@pytest.mark.parametrize("lead", C.LEADS)
@pytest.mark.parametrize("ft", C.FTS)
def test_partial_last_blocks_at_every_row_count(ft, lead):
    """last blocks of 1 .. 4095 words on both sides of the 8-row group boundaries, behind 0, 1, 3 or 8 whole blocks,
    accumulators at every word offset from a 16-byte boundary"""
    case = C.tails(ft, lead)
    members = list(range(len(case.sizes)))
    for m, mode in enumerate(MODES):
        for accumulate in (False, True):
            _decode_batch(case, 10, members, mode, lead + m, accumulate, f"lead {lead}", offsets=[(i + m) % 4 for i in members])


# ------------------------------------------------------------------------------ 3. capacity larger than the element
@pytest.mark.parametrize("ft", C.FTS)
def test_capacity_larger_than_the_element(ft):
    """the geometry comes from the capacity: tiles and half-waves past the element's end run, and must leave the words
    [size, capacity) of the accumulator alone"""
    import dietgpu_amd as dg

    case = C.capacity(ft)
    rows = _rows(case, 10)
    rules = list(C.CAPACITY_RULES.items())
    everything = list(range(len(case.sizes)))
    batches = [([i], [rule(case.sizes[i])], f"element {i} alone, capacity {name}") for i in everything for name, rule in rules]
    batches += [(everything, [rule(n) for n in case.sizes], f"all, capacity {name}") for name, rule in rules]
    for b, (members, caps, what) in enumerate(batches):
        mode, accumulate = MODES[b % 3], bool(b % 2)
        scale, fs = _factors_of(mode, len(members), b)
        accs = [Acc(cap) for cap in caps]
        for a, i in zip(accs, members):
            a.buf[a.lo : a.lo + a.n].fill_(int(SENTINEL2))
            if accumulate:
                a.view[: case.sizes[i]].copy_(torch.from_numpy(case.start[i]))
        status = torch.full((len(members),), 7, dtype=torch.uint8, device=_dev())
        sizes = torch.full((len(members),), -7, dtype=torch.int32, device=_dev())
        dg.decompress_data_accumulate([rows[i] for i in members], [a.view for a in accs], accumulate, None, status, sizes,
                                      dtype=C.DTYPE[ft], scale=scale)
        what2 = f"ft={ft} {mode} accumulate={accumulate} {what}"
        assert status.tolist() == [1] * len(members), what2
        assert sizes.tolist() == [case.sizes[i] for i in members], what2
        for k, (i, a) in enumerate(zip(members, accs)):
            got, n = a.bits(), case.sizes[i]
            _same(got[:n], _want(case, i, fs[k], accumulate), f"{what2}: element {i}")
            assert (got[n:].view(np.int32) == SENTINEL2).all(), f"{what2}: element {i}: words past its size were written"
            assert a.guards_intact(), f"{what2}: element {i}: guard words overwritten"


# -------------------------------------------------------------------------------------- 4. malformed descriptors
@pytest.mark.parametrize("name", list(C.MALFORMED_BATCHES))
@pytest.mark.parametrize("ft", C.FTS)
def test_a_malformed_member_fails_alone_and_keeps_its_accumulator(ft, name):
    """status 0 for the corrupted member, whose accumulator keeps every bit; both neighbours are exact"""
    import dietgpu_amd as dg

    tile_blocks, sizes, cap1 = C.MALFORMED_BATCHES[name]
    case = C.malformed(ft, name)
    rows = _rows(case, 10)
    caps = [sizes[0], cap1, sizes[2]]
    for c, (what, bad) in enumerate(C.corruptions(ft, case.archives(10)[1], sizes[1], tile_blocks)):
        mode, accumulate = MODES[c % 3], bool(c % 2)
        scale, fs = _factors_of(mode, 3, c)
        ins = [rows[0], torch.from_numpy(bad).to(_dev()), rows[2]]
        accs = [Acc(cap) for cap in caps]
        for k, a in enumerate(accs):
            a.view[: sizes[k]].copy_(torch.from_numpy(case.start[k]))
        before = accs[1].bits()
        status = torch.full((3,), 7, dtype=torch.uint8, device=_dev())
        out_sizes = torch.full((3,), -7, dtype=torch.int32, device=_dev())
        dg.decompress_data_accumulate(ins, [a.view for a in accs], accumulate, None, status, out_sizes, dtype=C.DTYPE[ft], scale=scale)
        what2 = f"ft={ft} {name}, {what}, {mode}, accumulate={accumulate}"
        assert status.tolist() == [1, 0, 1], what2
        assert out_sizes.tolist() == sizes, what2  # the header is valid in every case
        _same(accs[1].bits(), before, f"{what2}: the failing member's accumulator")
        for k in (0, 2):
            _same(accs[k].bits(), _want(case, k, fs[k], accumulate), f"{what2}: neighbour {k}")
        assert all(a.guards_intact() for a in accs), what2 + ": guard words overwritten"


# ----------------------------------------------------------------------------- 5. against the calls that exist today
@pytest.mark.parametrize("ft", C.FTS)
def test_store_with_a_host_factor_is_decode_reduce_of_one_source_with_that_scale(ft):
    import dietgpu_amd as dg

    case = C.staging(ft, 0)
    rows = _rows(case, 10)
    for f in FACTORS:
        ours = [Acc(n) for n in case.sizes]
        theirs = [Acc(n) for n in case.sizes]
        st = torch.zeros(len(rows), dtype=torch.uint8, device=_dev())
        dg.decompress_data_accumulate(rows, [a.view for a in ours], False, None, st, None, dtype=C.DTYPE[ft], scale=float(f))
        assert st.tolist() == [1] * len(rows)
        st.zero_()
        dg.decompress_data_reduce([[r] for r in rows], [a.view for a in theirs], False, None, st, None, dtype=C.DTYPE[ft], scale=float(f))
        assert st.tolist() == [1] * len(rows)
        for i, (a, b) in enumerate(zip(ours, theirs)):
            _same(a.bits(), b.bits(), f"ft={ft} factor {float(f)!r} element {i}: against decompress_data_reduce(scale=)")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ft", C.FTS)
def test_add_is_decode_accumulate_into_a_scratch_mul_and_add(ft, mode):
    import dietgpu_amd as dg

    case = C.staging(ft, 0)
    rows = _rows(case, 10)
    B = len(rows)
    scale, fs = _factors_of(mode, B, 1)
    ours = [Acc(n, fill=case.start[i]) for i, n in enumerate(case.sizes)]
    theirs = [Acc(n, fill=case.start[i]) for i, n in enumerate(case.sizes)]
    st = torch.zeros(B, dtype=torch.uint8, device=_dev())
    dg.decompress_data_accumulate(rows, [a.view for a in ours], True, None, st, None, dtype=C.DTYPE[ft], scale=scale)
    assert st.tolist() == [1] * B
    scratch = [torch.empty(n, dtype=torch.float32, device=_dev()) for n in case.sizes]
    st.zero_()
    dg.decompress_data_accumulate(rows, scratch, False, None, st, None, dtype=C.DTYPE[ft])
    assert st.tolist() == [1] * B
    for i, (s, a) in enumerate(zip(scratch, theirs)):
        s.mul_(torch.tensor(float(fs[i]), dtype=torch.float32, device=_dev()))
        a.view.add_(s)
    for i, (a, b) in enumerate(zip(ours, theirs)):
        _same(a.bits(), b.bits(), f"ft={ft} {mode} element {i}: against decode-accumulate + mul_ + add_")
        _same(a.bits(), _want(case, i, fs[i], True), f"ft={ft} {mode} element {i}: against the reference")


# ------------------------------------------------------------------------------------------- 6. particular factors
def _compress_words(ft, w):
    import dietgpu_amd as dg

    t = torch.from_numpy(w.view(C.SIGNED[ft]).copy()).view(C.DTYPE[ft]).to(_dev())
    comp, sizes, _ = dg.compress_data(True, [t], False, None)
    return comp[0, : int(sizes[0])]


def test_host_factor_one_is_the_plain_call_and_keeps_a_signalling_nan():
    import dietgpu_amd as dg

    w = np.resize(np.array([0x3F800000, 0x7F800001, 0xFFA00000, 0x00000001, 0x7FC00000, 0x40490FDB], dtype=np.uint32), C.BLK + 4097)
    row = _compress_words(A.FLOAT32, w)
    st = torch.zeros(1, dtype=torch.uint8, device=_dev())
    for one in (1.0, 1.0 + 1e-12):
        a = Acc(w.size)
        dg.decompress_data_accumulate([row], [a.view], False, None, st, None, dtype=torch.float32, scale=one)
        assert st.tolist() == [1]
        _same(a.bits(), w, f"host factor {one!r}: the bits of every word, signalling NaNs included")
        assert a.guards_intact()
    # the bare entry point forwards too
    a = Acc(w.size)
    used = ctypes.c_size_t(99)
    rc = dg.lib().dgpu_float_decode_accumulate_scaled(
        None, 0, ctypes.byref(used), A.FLOAT32, 10, 0, 1, (ctypes.c_void_p * 1)(row.data_ptr()), (ctypes.c_uint32 * 1)(row.numel()),
        (ctypes.c_void_p * 1)(a.view.data_ptr()), (ctypes.c_uint32 * 1)(w.size), 1.0, None, 0, ctypes.c_void_p(st.data_ptr()), None,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and used.value == 0, dg.lib().dgpu_last_error()
    torch.cuda.synchronize()
    _same(a.bits(), w, "dgpu_float_decode_accumulate_scaled with a host factor of 1.0f")
    # a DEVICE factor of 1 multiplies: every word that is not a NaN keeps its bits, a NaN stays a NaN
    a = Acc(w.size)
    dg.decompress_data_accumulate([row], [a.view], False, None, st, None, dtype=torch.float32,
                                  scale=torch.ones(1, dtype=torch.float32, device=_dev()))
    nan = A.is_nan(w)
    _same(a.bits()[~nan], w[~nan], "device factor 1.0")
    assert A.is_nan(a.bits())[nan].all()


@pytest.mark.parametrize("ft", C.FTS)
def test_device_factors_zero_infinity_and_nan(ft):
    """a 4097-word element with zeros of both signs, denormals and extremes: where the reference has a NaN the result is
    a NaN, every other word is the reference's"""
    import dietgpu_amd as dg

    if ft == A.FLOAT32:
        pats = [0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x807FFFFF, 0x00800000, 0x3F800000, 0xBF800001, 0x40490FDB]
    elif ft == A.FLOAT16:
        pats = [0x0000, 0x8000, 0x7BFF, 0xFBFF, 0x0001, 0x83FF, 0x0400, 0x3C00, 0xBC01, 0x4248]
    else:
        pats = [0x0000, 0x8000, 0x7F7F, 0xFF7F, 0x0001, 0x807F, 0x0080, 0x3F80, 0xBF81, 0x4049]
    w = np.resize(np.array(pats, dtype=C.WORD[ft]), 4097)
    row = _compress_words(ft, w)
    start = C.random_acc(w.size, 77)
    start[::7] = -0.0
    st = torch.zeros(1, dtype=torch.uint8, device=_dev())
    for factor in (0.0, -0.0, float("inf"), float("-inf"), float("nan")):
        for accumulate in (False, True):
            want = A.accum_scaled_ref(w, ft, factor, C.bits(start) if accumulate else None)
            a = Acc(w.size, fill=start if accumulate else None)
            dg.decompress_data_accumulate([row], [a.view], accumulate, None, st, None, dtype=C.DTYPE[ft],
                                          scale=torch.tensor([factor], dtype=torch.float32, device=_dev()))
            what = f"ft={ft} device factor {factor!r} accumulate={accumulate}"
            assert st.tolist() == [1], what
            got, nan = a.bits(), A.is_nan(want)
            assert A.is_nan(got)[nan].all(), f"{what}: a NaN of the reference is not a NaN"
            _same(got[~nan], want[~nan], what)
            assert a.guards_intact(), what
            if str(factor) == "0.0" and accumulate:  # finite accumulators keep their bits; -0 + a +0 product = +0
                acc, positive = C.bits(start), (w >> (31 if ft == A.FLOAT32 else 15)) == 0
                assert not nan.any() and (want[acc != 0x80000000] == acc[acc != 0x80000000]).all()
                assert (want[(acc == 0x80000000) & positive] == 0).all() and ((acc == 0x80000000) & positive).any()


# ---------------------------------------------------------------------------------------------------- 7. capture
def test_graph_replay_follows_the_factor_in_memory():
    """one linear capture of a call with a device factor (a host synchronisation inside the call would end the capture
    with an error); replayed after the factor tensor is overwritten, the accumulators follow the NEW value"""
    import dietgpu_amd as dg

    ft = A.BFLOAT16
    case = C.staging(ft, 0)
    members = [0, 2]
    rows = [_rows(case, 10)[i] for i in members]
    accs = [Acc(case.sizes[i], fill=case.start[i]) for i in members]
    views = [a.view for a in accs]
    status = torch.zeros(2, dtype=torch.uint8, device=_dev())
    scale = torch.tensor([float(THIRD)], dtype=torch.float32, device=_dev())

    def call():  # (dtype given: reading the header would synchronise, which a capture cannot hold)
        dg.decompress_data_accumulate(rows, views, True, None, status, None, dtype=torch.bfloat16, scale=scale)

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
            for a, i in zip(accs, members):
                a.view.copy_(torch.from_numpy(case.start[i]))
            status.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert status.tolist() == [1, 1]
            for k, i in enumerate(members):
                _same(accs[k].bits(), _want(case, i, factor, True), f"replay with {float(factor)!r} in the factor tensor, element {i}")
                assert accs[k].guards_intact()
    finally:
        del graph
        dg.lib().dgpu_release_graph_state()
