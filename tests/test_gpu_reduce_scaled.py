"""Scaled decode-reduce on the GPU (dgpu_float_decode_reduce_scaled, k_ans_decode_reduce_mixed_scaled): every successful
member is left with acc[i] = fl32(U[i] * scale), U being, bit for bit, what the unscaled call leaves -- one IEEE float32
multiply on the last source's store.

Expected values are built on the host: tests/reduce_cases.py's expected(S, accumulate) times np.float32(scale) in
float32.  No product of these cases is NaN (infinities and float32 denormals do occur), so every comparison is on uint32
views, every word of it.  Where NaNs are planted on purpose the comparison is GPU against GPU and no NaN bits are
asserted: payload and sign of a generated NaN are the platform's."""
import ctypes

import numpy as np
import pytest
import torch

import accum_cases as C
import oracle as O
import reduce_cases as R
from test_gpu_accumulate import Acc, _dev
from test_gpu_reduce import _gpu, _rows, _same, _upload
from test_gpu_reduce_mixed import _ins, _raw, _raws

pytestmark = pytest.mark.gpu

THIRD = 1.0 / 3.0
SCALES = (THIRD, 0.5, -3.0)


def scaled(want, scale):
    """fl32(want * fl32(scale)), one multiply per word"""
    with np.errstate(over="ignore", under="ignore"):
        out = (np.ascontiguousarray(want, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    assert not np.isnan(out).any()
    return out


def patterns(S):
    """raw sources: none, the first, the last, all"""
    seen, out = set(), []
    for name, p in (("none", ()), ("first", (0,)), ("last", (S - 1,)), ("all", tuple(range(S)))):
        if p not in seen:
            seen.add(p)
            out.append((name, p))
    return out


def _scaled_and_check(src, rows, raws, S, prob_bits, members, accumulate, raw_at, scale, what, offsets=None):
    """one scaled call for `members` with the first S sources, those at `raw_at` raw: no temp memory, status, sizes,
    every accumulator word, the guards"""
    import dietgpu_amd as dg

    B = len(members)
    accs = [Acc(src.sizes[i], offsets[k] if offsets else 0, fill=src.start[i] if accumulate else None) for k, i in enumerate(members)]
    status = torch.full((B,), 7, dtype=torch.uint8, device=_dev())
    sizes = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    f = dg.decompress_data_reduce_mixed if raw_at else dg.decompress_data_reduce
    used = f(_ins(rows, raws, S, members, raw_at), [a.view for a in accs], accumulate, None, status, sizes, prob_bits=prob_bits,
             dtype=C.DTYPE[src.ft], scale=scale)
    what = f"ft={src.ft} probBits={prob_bits} S={S} accumulate={accumulate} raw at {list(raw_at)} scale={scale} {what}"
    assert used == 0, what
    assert status.tolist() == [1] * B, what
    assert sizes.tolist() == [src.sizes[i] for i in members], what
    want = src.expected(S, bool(accumulate))
    for k, i in enumerate(members):
        _same(accs[k].bits(), C.bits(scaled(want[i], scale)), f"{what}: member {k} ({src.sizes[i]} words)")
        assert accs[k].guards_intact(), f"{what}: member {k}: guard words overwritten"


# ------------------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("ft", C.FTS)
def test_scaled_equals_the_host_product(ft, S, accumulate):
    """the staging shapes (16- and 4-block tiles, whole, ring, mixed and boundary waves, partial last blocks); S == 1 runs
    the reducing kernel too (decode-accumulate does not scale)"""
    src = R.staging(ft)
    rows, raws = _rows(src, "staging", 10), _raws(src, "staging")
    members = list(range(len(src.sizes)))
    for scale in SCALES:
        for name, raw_at in patterns(S):
            _scaled_and_check(src, rows, raws, S, 10, members, accumulate, raw_at, scale, f"staging shapes, raw {name}")


@pytest.mark.parametrize("ft,prob_bits", [(O.BFLOAT16, 9), (O.FLOAT16, 11), (O.FLOAT32, 11)])
def test_other_table_precisions(ft, prob_bits):
    src = R.staging(ft)
    rows, raws = _rows(src, "staging", prob_bits), _raws(src, "staging")
    members = list(range(len(src.sizes)))
    for accumulate in (0, 1):
        _scaled_and_check(src, rows, raws, 2, prob_bits, members, accumulate, (), THIRD, "staging shapes")
        _scaled_and_check(src, rows, raws, 2, prob_bits, members, accumulate, (1,), THIRD, "staging shapes")


@pytest.mark.parametrize("lead", [0, 3])
@pytest.mark.parametrize("ft", C.FTS)
def test_partial_last_blocks(ft, lead):
    """every length of a last block: the row-wise store path; accumulators at word offsets 0..3"""
    src = R.tails(ft, lead)
    rows, raws = _rows(src, f"tails{lead}", 10), _raws(src, f"tails{lead}")
    members = list(range(len(src.sizes)))
    for accumulate in (0, 1):
        for raw_at in ((), (1,)):
            _scaled_and_check(src, rows, raws, 2, 10, members, accumulate, raw_at, THIRD, f"lead {lead}", offsets=[i % 4 for i in members])


@pytest.mark.parametrize("ft", C.FTS)
def test_workgroup_orders_and_work_lists(ft):
    import dietgpu_amd as dg

    L = dg.lib()
    B = 13
    for tile_blocks in C.ORDER_GEOMETRIES:
        src = R.orders(ft, B, tile_blocks)
        rows, raws = _rows(src, f"orders{B}x{tile_blocks}", 10), _raws(src, f"orders{B}x{tile_blocks}")
        members = list(range(B))
        assert -(-max(src.sizes) // C.BLK) == C.ORDER_GEOMETRIES[tile_blocks][1]  # this geometry, two tiles per member
        for order in (0, 1, 2):
            L.dgpu_debug_set_decoder_order(order)
            try:
                _scaled_and_check(src, rows, raws, 2, 10, members, order % 2, (), -3.0, f"order {order}, {tile_blocks}-block tiles")
            finally:
                L.dgpu_debug_set_decoder_order(-1)
        for lists in (1, 0):
            L.dgpu_debug_set_work_lists(lists)
            try:
                for accumulate, raw_at in ((0, (1,)), (1, ())):
                    _scaled_and_check(src, rows, raws, 2, 10, members, accumulate, raw_at, THIRD, f"work lists {lists}, {tile_blocks}-block tiles")
            finally:
                L.dgpu_debug_set_work_lists(-1)


# --------------------------------------------------------------------------------------------------------- scale 1.0
@pytest.mark.parametrize("ft", C.FTS)
def test_scale_one_is_the_unscaled_call(ft):
    """S == 1, accumulate == 0 on words of any bits: what is stored is the widened word -- no multiply runs, so a
    signalling NaN keeps its bits, as in decompress_data_accumulate, which this call then is"""
    import dietgpu_amd as dg

    n = 2 * C.BLK + 777
    w = R.any_bits(n, 300)
    w = w if ft == O.FLOAT32 else (w >> 16).astype(np.uint16)
    exp = C.EXP_MASK[ft]
    w[5] = exp | 1  # a signalling NaN of the type
    archive = _upload(O.float_compress(ft, w, 10))

    def run(f, **kw):
        a = Acc(n)
        status = torch.zeros(1, dtype=torch.uint8, device=_dev())
        f(a.view, status, **kw)
        assert status.tolist() == [1] and a.guards_intact()
        return a.bits()

    plain = run(lambda acc, st: dg.decompress_data_accumulate([archive], [acc], False, None, st, None, dtype=C.DTYPE[ft]))
    for f in (dg.decompress_data_reduce, dg.decompress_data_reduce_mixed):
        for scale in (1.0, 1, 1.0 + 2.0 ** -30, None):
            got = run(lambda acc, st: f([[archive]], [acc], False, None, st, None, dtype=C.DTYPE[ft], scale=scale))
            _same(got, plain, f"ft={ft} scale={scale}: against decompress_data_accumulate")
    # ... through the C ABI with scale 1.0f and sourceKind NULL
    a = Acc(n)
    used = ctypes.c_size_t(99)
    rc = dg.lib().dgpu_float_decode_reduce_scaled(
        None, 0, ctypes.byref(used), ft, 10, 0, 1, 1, (ctypes.c_void_p * 1)(archive.data_ptr()), (ctypes.c_uint32 * 1)(archive.numel()), None,
        1.0, (ctypes.c_void_p * 1)(a.view.data_ptr()), (ctypes.c_uint32 * 1)(n), None, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and used.value == 0, dg.lib().dgpu_last_error()
    _same(a.bits(), plain, f"ft={ft}: dgpu_float_decode_reduce_scaled with scale 1")
    # the widening is a matter of bits for bfloat16 and float32, and exact for every float16 word that is not a NaN
    if ft == O.FLOAT32:
        _same(plain, w, "float32 words are stored as they are")
    elif ft == O.BFLOAT16:
        _same(plain, w.astype(np.uint32) << 16, "bfloat16 words are stored shifted")
    else:
        nan = (w & 0x7FFF) > exp
        assert nan.any()
        _same(plain[~nan], C.bits(C.widen(ft, w))[~nan], "float16 words that are not NaN")
        assert np.isnan(plain.view(np.float32)[nan]).all()


# ------------------------------------------------------------------------------------- the old contents are covered too
def test_the_scale_covers_the_old_accumulator_contents():
    """accumulator 1.0, one bfloat16 source of 2.0, accumulate, scale 0.25: 0.75 everywhere (1.5 would be acc + x * scale)"""
    import dietgpu_amd as dg

    ft, n = O.BFLOAT16, R.ORDER_WORDS
    two = R.constant_words(ft, 2.0)
    archive, raw = _upload(O.float_compress(ft, two, 10)), _raw(ft, two)
    for f, source in ((dg.decompress_data_reduce, archive), (dg.decompress_data_reduce_mixed, raw)):
        a = Acc(n, fill=np.ones(n, np.float32))
        status = torch.zeros(1, dtype=torch.uint8, device=_dev())
        f([[source]], [a.view], True, None, status, None, dtype=C.DTYPE[ft], scale=0.25)
        assert status.tolist() == [1]
        got = a.bits().view(np.float32)
        assert (got == np.float32(0.75)).all(), got[:4]
        assert a.guards_intact()


# -------------------------------------------------------------------------------------------------- any bit pattern
@pytest.mark.parametrize("ft", C.FTS)
def test_any_bit_pattern_scales_like_a_multiply_of_the_sum(ft):
    """sources of random bits with +-inf and NaN planted: the scaled call against the unscaled call followed by mul_ with
    a 0-dim float32 tensor, GPU against GPU.  Words that are not NaN match bit for bit; NaN words are NaN in both."""
    import dietgpu_amd as dg

    n, S = 2 * C.BLK + 777, 3
    exp, low = C.EXP_MASK[ft], C.EXP_LOW[ft]
    words = []
    for s in range(S):
        w = R.any_bits(n, 100 + s)
        w = w if ft == O.FLOAT32 else (w >> 16).astype(np.uint16)
        specials = [exp, exp | (exp + low), 1, exp | 5]  # +inf, -inf, the smallest denormal, a NaN with a payload
        for k in range(len(specials)):
            w[C.BLK - 2 + k] = specials[(k + s) % len(specials)]
        # (rotated, the infinities above meet each other or a NaN; these two survive the sum and are scaled)
        w[C.BLK + 10], w[C.BLK + 11] = specials[0], specials[1]
        words.append(w)
    archives = [_upload(O.float_compress(ft, w, 10)) for w in words]
    raws = [_raw(ft, w) for w in words]
    start = R.any_bits(n, 200)
    start[C.BLK + 10 : C.BLK + 12] = np.float32(1.0).view(np.uint32)
    for accumulate in (0, 1):
        for scale in (THIRD, -3.0):
            def run(ins, **kw):
                a = Acc(n)
                a.view.view(torch.int32).copy_(torch.from_numpy(start.view(np.int32)))
                status = torch.zeros(1, dtype=torch.uint8, device=_dev())
                dg.decompress_data_reduce_mixed([ins], [a.view], accumulate, None, status, None, dtype=C.DTYPE[ft], **kw)
                assert status.tolist() == [1]
                return a

            ref = run(archives)
            ref.view.mul_(torch.tensor(scale, dtype=torch.float32, device=_dev()))
            want = ref.bits()
            nan = np.isnan(want.view(np.float32))
            assert nan.any() and np.isinf(want.view(np.float32)).any()
            for raw_at in ((), (2,), (0, 1, 2)):
                a = run([raws[s] if s in raw_at else archives[s] for s in range(S)], scale=scale)
                got = a.bits()
                what = f"ft={ft} accumulate={accumulate} scale={scale} raw at {list(raw_at)}"
                _same(got[~nan], want[~nan], what + ": the words that are not NaN")
                assert np.isnan(got.view(np.float32)[nan]).all(), what
                assert a.guards_intact(), what


# --------------------------------------------------------------------------------------------------- all or nothing
@pytest.mark.parametrize("ft", C.FTS)
def test_a_member_with_a_malformed_source_keeps_every_bit(ft):
    """three members, three sources each; a source of the middle member is malformed: status [1, 0, 1], the middle
    accumulator (any bits) as it was, the neighbours summed and scaled"""
    import dietgpu_amd as dg

    name = "two 4-block tiles"
    tile_blocks, sizes, cap1 = C.MALFORMED_BATCHES[name]
    src = R.malformed(ft, name)
    rows, raws = _rows(src, "malformed " + name, 10), _raws(src, "malformed " + name)
    good = src.archives(10)[1][1]
    corruptions = list(C.corruptions(ft, good, sizes[1], tile_blocks))
    for what, bad in (corruptions[0], corruptions[-1]):
        for accumulate, raw_neighbours in ((0, False), (1, True)):
            ins = [[raws[0][0] if raw_neighbours else rows[0][0], rows[1][0], rows[2][0]], [rows[0][1], _upload(bad), rows[2][1]],
                   [rows[0][2], rows[1][2], raws[2][2] if raw_neighbours else rows[2][2]]]
            caps = [sizes[0], cap1, sizes[2]]
            fills = [R.finite_bits(cap, 10 * k + accumulate) for k, cap in enumerate(caps)]
            middle = R.any_bits(cap1, 3 + accumulate)
            assert np.isnan(middle.view(np.float32)).any()
            accs = [Acc(cap, fill=f) for cap, f in zip(caps, fills)]
            accs[1].view.view(torch.int32).copy_(torch.from_numpy(middle.view(np.int32)))
            status = torch.full((3,), 7, dtype=torch.uint8, device=_dev())
            out_sizes = torch.full((3,), -7, dtype=torch.int32, device=_dev())
            f = dg.decompress_data_reduce_mixed if raw_neighbours else dg.decompress_data_reduce
            f(ins, [a.view for a in accs], accumulate, None, status, out_sizes, dtype=C.DTYPE[ft], scale=THIRD)
            what2 = f"ft={ft} {name}, source 1: {what}, accumulate={accumulate}"
            assert status.tolist() == [1, 0, 1], what2
            assert out_sizes.tolist() == list(sizes), what2
            _same(accs[1].bits(), middle, f"{what2}: the failing member's accumulator")
            for k in (0, 2):
                want = R.reduce_expected(fills[k], [src.wide[s][k] for s in range(3)], bool(accumulate))
                with np.errstate(invalid="ignore"):
                    assert not np.isnan(want).any()
                _same(accs[k].bits(), C.bits(scaled(want, THIRD)), f"{what2}: neighbour {k}")
            assert all(a.guards_intact() for a in accs), what2 + ": guard words overwritten"


# ------------------------------------------------------------------------------------------------------------ routes
def test_routes_agree_and_calls_that_differ_in_scale_share_the_batch():
    """the ctypes route, the torch op and the C ABI itself (sourceKind given and NULL); the same batch under three scales
    in turn: the scale is an argument of the launch, not of the cached batch"""
    import dietgpu_amd as dg

    ft, S = C.FTS[1], 3
    src = R.staging(ft)
    rows, raws = _rows(src, "staging", 10), _raws(src, "staging")
    B = len(src.sizes)
    members = list(range(B))
    want = src.expected(S, True)
    if dg.ops._fast_ops(10) is not None:
        assert hasattr(torch.ops.dietgpu_amd, "decompress_data_reduce_scaled")
    try:
        for route in (False, True):
            dg.prefer_torch_ops(route)
            for scale in (THIRD, 0.5, THIRD):
                accs = [Acc(n, fill=src.start[i]) for i, n in enumerate(src.sizes)]
                assert dg.decompress_data_reduce_mixed(_ins(rows, raws, S, members, (1,)), [a.view for a in accs], True, scale=scale) == 0
                for k in members:
                    _same(accs[k].bits(), C.bits(scaled(want[k], scale)), f"torch ops {route}, scale {scale}: member {k}")
    finally:
        dg.prefer_torch_ops(True)
    for raw_at in ((1,), ()):
        flat = [t for member in _ins(rows, raws, S, members, raw_at) for t in member]
        kinds = [0 if t.dtype == torch.uint8 else 1 for t in flat]
        accs = [Acc(n, fill=src.start[i]) for i, n in enumerate(src.sizes)]
        used = ctypes.c_size_t(99)
        rc = dg.lib().dgpu_float_decode_reduce_scaled(
            None, 0, ctypes.byref(used), ft, 10, 1, B, S, (ctypes.c_void_p * (B * S))(*[r.data_ptr() for r in flat]),
            (ctypes.c_uint32 * (B * S))(*[r.numel() * r.element_size() for r in flat]), (ctypes.c_uint8 * (B * S))(*kinds) if raw_at else None,
            -3.0, (ctypes.c_void_p * B)(*[a.view.data_ptr() for a in accs]), (ctypes.c_uint32 * B)(*src.sizes), None, None,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0 and used.value == 0, dg.lib().dgpu_last_error()
        for k in members:
            _same(accs[k].bits(), C.bits(scaled(want[k], -3.0)), f"C ABI, raw at {list(raw_at)}: member {k}")


# ------------------------------------------------------------------------------------------------------------- graph
def test_graph_replay_stores_the_scaled_sum_again():
    """a warm call, the same call captured, two replays with accumulate off: the same bits each time"""
    import dietgpu_amd as dg

    ft, S, members = C.FTS[1], 3, [0, 1, 5]
    src = R.staging(ft)
    rows, raws = _rows(src, "staging", 10), _raws(src, "staging")
    ins = _ins(rows, raws, S, members, (1,))
    accs = [Acc(src.sizes[i]) for i in members]
    views = [a.view for a in accs]
    status = torch.zeros(len(members), dtype=torch.uint8, device=_dev())

    def call():  # (dtype given: nothing synchronises)
        dg.decompress_data_reduce_mixed(ins, views, False, None, status, None, dtype=C.DTYPE[ft], scale=THIRD)

    want = src.expected(S, False)
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call()  # the warm call: makes the parameter block resident
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            call()
        torch.cuda.synchronize()
        for replay in range(2):
            for a in accs:
                a.view.fill_(float("nan"))
            status.fill_(7)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert status.tolist() == [1] * len(members)
            for a, i in zip(accs, members):
                _same(a.bits(), C.bits(scaled(want[i], THIRD)), f"replay {replay}: member {i}")
                assert a.guards_intact()
        del graph
    finally:
        dg.lib().dgpu_release_graph_state()
