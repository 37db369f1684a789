"""The norm outputs of decode-reduce on the GPU (dgpu_float_decode_reduce_norm, k_ans_decode_reduce_mixed_norm): per
member, out_sumsq = the sum of squares (float64) of the finite float32 words the call leaves in the accumulator and
out_nonfinite = the number of words that are inf or NaN -- of the words the sources state, after the last add and after
the multiply by the scale, with accumulate including the old contents.

Expected values come from tests/norm_ref.py: math.fsum of the exact float64 squares of the expected words (the host sums
of tests/reduce_cases.py), so the bound of n * 2**-52 is spent on the kernel alone; the count is exact.  Everything else
the call leaves must be, bit for bit, what the same call without the two outputs leaves."""
import ctypes

import numpy as np
import pytest
import torch

import accum_cases as C
import norm_ref as N
import oracle as O
import reduce_cases as R
from test_gpu_accumulate import Acc, _dev
from test_gpu_reduce import _gpu, _rows, _same, _upload
from test_gpu_reduce_mixed import _ins, _raw, _raws

pytestmark = pytest.mark.gpu

THIRD = 1.0 / 3.0


def scaled(want, scale):
    if scale is None:
        return np.ascontiguousarray(want, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return (np.ascontiguousarray(want, dtype=np.float32) * np.float32(scale)).astype(np.float32)


def _same_words(got, want, what):
    """uint32 views; NaN words must be NaN in both, every other word equal bit for bit"""
    nan = np.isnan(want.view(np.float32))
    _same(got[~nan], want[~nan], what + ": the words that are not NaN")
    assert np.isnan(got.view(np.float32)[nan]).all(), what


class Norm:
    def __init__(self, n):
        self.sumsq = torch.full((n,), -1.0, dtype=torch.float64, device=_dev())
        self.nonfinite = torch.full((n,), -7, dtype=torch.int32, device=_dev())


def _call(f, ins, src, members, accumulate, scale, norm, prob_bits=10, offsets=None, temp=None, caps=None, fills=None):
    accs = [Acc(caps[k] if caps else src.sizes[i], offsets[k] if offsets else 0,
                fill=(fills[k] if fills else src.start[i]) if accumulate or fills else None) for k, i in enumerate(members)]
    B = len(members)
    status = torch.full((B,), 7, dtype=torch.uint8, device=_dev())
    sizes = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    kw = {} if norm is None else {"out_sumsq": norm.sumsq, "out_nonfinite": norm.nonfinite}
    used = f(ins, [a.view for a in accs], accumulate, temp, status, sizes, prob_bits=prob_bits, dtype=C.DTYPE[src.ft], scale=scale, **kw)
    return accs, status, sizes, used


def _check_case(src, tag, S, accumulate, scale, raw_at=(), offsets=None, prob_bits=10):
    import dietgpu_amd as dg

    rows, raws = _rows(src, tag, prob_bits), _raws(src, tag)
    members = list(range(len(src.sizes)))
    B = len(members)
    ins = _ins(rows, raws, S, members, raw_at)
    f = dg.decompress_data_reduce_mixed if raw_at else dg.decompress_data_reduce
    norm = Norm(B)
    accs, status, sizes, used = _call(f, ins, src, members, accumulate, scale, norm, prob_bits, offsets)
    plain, status0, sizes0, used0 = _call(f, ins, src, members, accumulate, scale, None, prob_bits, offsets)
    what = f"{tag} ft={src.ft} S={S} accumulate={accumulate} scale={scale} raw at {list(raw_at)}"
    assert used0 == 0 and 0 < used <= dg.lib().dgpu_float_reduce_norm_temp_bytes(src.ft, B, max(src.sizes), 0), (what, used)
    assert status.tolist() == status0.tolist() == [1] * B, what
    assert sizes.tolist() == sizes0.tolist() == list(src.sizes), what
    want = src.expected(S, bool(accumulate))
    sumsq, nonfinite = norm.sumsq.tolist(), norm.nonfinite.tolist()
    for k in members:
        words = scaled(want[k], scale)
        _same(accs[k].bits(), plain[k].bits(), f"{what}: member {k} against the call without the outputs")
        _same_words(accs[k].bits(), C.bits(words), f"{what}: member {k} against the host")
        assert accs[k].guards_intact(), what
        N.check(sumsq[k], nonfinite[k], words, f"{what}: member {k}")


# ------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("scale", [None, THIRD])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("ft", C.FTS)
def test_values_on_the_staging_and_partial_block_cases(ft, S, accumulate, scale):
    """staging: 16-block tiles, several per member; the partial-last-block cases: single-block members (lead 0) in 4-block
    tiles, accumulators at word offsets 0..3"""
    _check_case(R.staging(ft), "staging", S, accumulate, scale)
    if S <= 2:
        for lead in (0, 3):
            src = R.tails(ft, lead)
            _check_case(src, f"tails{lead}", S, accumulate, scale, offsets=[i % 4 for i in range(len(src.sizes))])


@pytest.mark.parametrize("ft", C.FTS)
def test_a_raw_row_as_the_last_and_as_the_first_source(ft):
    for raw_at in ((2,), (0,), (0, 1, 2)):
        for accumulate, scale in ((0, THIRD), (1, None)):
            _check_case(R.staging(ft), "staging", 3, accumulate, scale, raw_at=raw_at)
    src = R.tails(ft, 0)
    _check_case(src, "tails0", 2, 0, None, raw_at=(1,), offsets=[i % 4 for i in range(len(src.sizes))])


@pytest.mark.parametrize("ft,prob_bits", [(O.BFLOAT16, 9), (O.FLOAT16, 11), (O.FLOAT32, 11)])
def test_other_table_precisions(ft, prob_bits):
    _check_case(R.staging(ft), "staging", 2, 1, THIRD, prob_bits=prob_bits)


# ----------------------------------------------------------------------------------------------------- planted words
def _planted(ft):
    """two sources of two blocks and a 37-word tail, and a starting accumulator: -> (words [2], start, positions)"""
    n = 2 * C.BLK + 37
    w = [C.words(ft, "cc", 37, "c", seed=71000 + s) for s in range(2)]  # magnitudes around one
    exp, low = C.EXP_MASK[ft], C.EXP_LOW[ft]
    sign = exp + low
    pos = {"+inf": 5, "-inf": C.BLK - 1, "nan": C.BLK + 64, "denormal": 2 * C.BLK + 36, "big0": 100, "big1": 2 * C.BLK + 3, "sum": 2 * C.BLK - 7}
    for p in pos.values():
        w[0][p] = w[1][p] = 0
    w[0][pos["+inf"]] = exp
    w[1][pos["-inf"]] = exp | sign
    w[0][pos["nan"]] = exp | 5
    w[1][pos["denormal"]] = 1
    start = (R.finite_bits(n, 5).view(np.uint32) & np.uint32(0xBFFFFFFF)).view(np.float32).copy()  # |x| < 2
    for p in pos.values():
        start[p] = 0.0
    # two words near the largest finite float32: their squares overflow float32 (in the accumulator for every type, and in
    # the sources too where the type reaches that far)
    start[pos["big0"]], start[pos["big1"]] = np.float32(3.0e38), np.float32(-3.2e38)
    if ft == O.FLOAT16:
        w[0][pos["sum"]] = int(np.float16(40000.0).view(np.uint16))
        w[1][pos["sum"]] = int(np.float16(30000.0).view(np.uint16))
    return w, start, pos


@pytest.mark.parametrize("ft", C.FTS)
def test_planted_words(ft):
    """+inf, -inf and a NaN are counted and left out of the sum; a denormal is not counted (its square is seen in the sum
    by test_denormals_are_finite_words_and_their_squares_are_summed, not beside these large words); two words near the largest
    finite float32 give a finite float64 where a float32 accumulation gives inf; float16: 40000 + 30000 = 70000 is a
    finite float32 word here (reduce-compress counts its float16 rounding as non-finite)"""
    import dietgpu_amd as dg

    w, start, pos = _planted(ft)
    n = w[0].size
    archives = [_upload(O.float_compress(ft, x, 10)) for x in w]
    raws = [_raw(ft, x) for x in w]
    wide = [C.widen(ft, x) for x in w]
    for ins in ([archives[0], archives[1]], [archives[0], raws[1]]):
        a = Acc(n, fill=start)
        norm = Norm(1)
        status = torch.zeros(1, dtype=torch.uint8, device=_dev())
        dg.decompress_data_reduce_mixed([ins], [a.view], True, None, status, None, dtype=C.DTYPE[ft], out_sumsq=norm.sumsq, out_nonfinite=norm.nonfinite)
        assert status.tolist() == [1]
        with np.errstate(invalid="ignore", over="ignore"):
            want = R.reduce_expected(start, wide, True)
        assert np.isnan(want[pos["nan"]]) and np.isposinf(want[pos["+inf"]]) and np.isneginf(want[pos["-inf"]])
        assert want[pos["denormal"]] != 0 and want[pos["big0"]] == np.float32(3.0e38)
        _same_words(a.bits(), C.bits(want), f"ft={ft}: the accumulator")
        exact, bad, _ = N.stats(want)
        with np.errstate(over="ignore"):
            assert np.isinf(np.sum(np.square(want[np.isfinite(want)], dtype=np.float32), dtype=np.float32))  # what float32 makes of it
        assert bad == 3 and np.isfinite(exact) and exact > 1.9e77
        if ft == O.FLOAT16:
            assert want[pos["sum"]] == np.float32(70000.0)
        N.check(norm.sumsq.item(), norm.nonfinite.item(), want, f"ft={ft} planted words")


def _denormal_words(ft):
    """a block and a 37-word tail of zeros with denormals of the type planted (float16: its denormals are small float32
    normals; bfloat16 and float32: float32 denormals), and nothing large beside them"""
    n = C.BLK + 37
    w = np.zeros(n, C.WORD[ft])
    low = C.EXP_LOW[ft]
    sign = C.EXP_MASK[ft] + low
    planted = [1, low - 1, sign | 1, low >> 1, sign | (low - 1), 3]
    for k, v in enumerate(planted):
        w[[0, 31, 32, 2049, C.BLK - 1, C.BLK + 36][k]] = v
    return w


@pytest.mark.parametrize("ft", C.FTS)
def test_denormals_are_finite_words_and_their_squares_are_summed(ft):
    """a member that holds nothing but zeros and denormals: a kernel that flushed them would report 0.0"""
    import dietgpu_amd as dg

    w = _denormal_words(ft)
    n = w.size
    zeros = np.zeros(n, C.WORD[ft])
    wide = C.widen(ft, w)
    want_sq, bad, _ = N.stats(wide)
    assert bad == 0 and 0.0 < want_sq < 1e-6 and np.count_nonzero(wide) == 6
    sources = {"archive": _upload(O.float_compress(ft, w, 10)), "raw": _raw(ft, w)}
    others = {"archive": _upload(O.float_compress(ft, zeros, 10)), "raw": _raw(ft, zeros)}
    for ins in (["archive"], ["raw"], ["archive", "raw"], ["raw", "archive"]):
        for accumulate in (0, 1):
            a = Acc(n, fill=np.zeros(n, np.float32))
            norm = Norm(1)
            status = torch.zeros(1, dtype=torch.uint8, device=_dev())
            rows = [sources[ins[0]]] + [others[k] for k in ins[1:]]
            dg.decompress_data_reduce_mixed([rows], [a.view], accumulate, None, status, None, dtype=C.DTYPE[ft], out_sumsq=norm.sumsq,
                                            out_nonfinite=norm.nonfinite)
            assert status.tolist() == [1]
            _same(a.bits(), C.bits(wide), f"ft={ft} {ins} accumulate={accumulate}: the accumulator")
            N.check(norm.sumsq.item(), norm.nonfinite.item(), wide, f"ft={ft} {ins} accumulate={accumulate} denormals")


# ------------------------------------------------------------------------------------------------------------ prefix
@pytest.mark.parametrize("ft", C.FTS)
def test_only_the_words_the_sources_state_are_measured(ft):
    """capacities larger than the members: the words behind the stated ones are infinities and NaNs that stay where they
    are and are not measured"""
    import dietgpu_amd as dg

    src = R.staging(ft)
    rows = _rows(src, "staging", 10)
    members = [1, 5, 0]
    extra = [5000, 1, 3 * C.BLK]
    caps = [src.sizes[i] + e for i, e in zip(members, extra)]
    fills = []
    for k, i in enumerate(members):
        f = np.full(caps[k], np.inf, np.float32)
        f[src.sizes[i] + 0 :: 2] = np.nan
        f[: src.sizes[i]] = src.start[i]
        fills.append(f)
    for accumulate in (0, 1):
        norm = Norm(3)
        accs, status, sizes, _ = _call(dg.decompress_data_reduce, [[rows[s][i] for s in range(2)] for i in members], src, members, accumulate, THIRD,
                                       norm, caps=caps, fills=fills)
        assert status.tolist() == [1, 1, 1] and sizes.tolist() == [src.sizes[i] for i in members]
        want = src.expected(2, bool(accumulate))
        for k, i in enumerate(members):
            got = accs[k].bits()
            _same(got[: src.sizes[i]], C.bits(scaled(want[i], THIRD)), f"ft={ft}: member {k}")
            _same_words(got[src.sizes[i] :], C.bits(fills[k][src.sizes[i] :]), f"ft={ft}: member {k} behind the stated words")
            N.check(norm.sumsq[k].item(), norm.nonfinite[k].item(), scaled(want[i], THIRD), f"ft={ft} accumulate={accumulate} prefix member {k}")


# --------------------------------------------------------------------------------------------- failed and empty members
@pytest.mark.parametrize("ft", C.FTS)
def test_a_failed_member_and_an_empty_member_get_zeros(ft):
    import dietgpu_amd as dg

    name = "two 4-block tiles"
    tile_blocks, sizes, cap1 = C.MALFORMED_BATCHES[name]
    src = R.malformed(ft, name)
    rows = _rows(src, "malformed " + name, 10)
    good = src.archives(10)[1][1]
    corruptions = list(C.corruptions(ft, good, sizes[1], tile_blocks))
    empty = _gpu(("empty", ft), lambda: _upload(O.float_compress(ft, np.zeros(0, C.WORD[ft]), 10)))
    for what, bad in (corruptions[0], corruptions[-1]):
        for accumulate in (0, 1):
            ins = [[rows[s][0] for s in range(3)], [rows[0][1], _upload(bad), rows[2][1]], [empty] * 3, [rows[s][2] for s in range(3)]]
            caps = [sizes[0], cap1, 0, sizes[2]]
            fills = [R.finite_bits(cap, 10 * k + accumulate) for k, cap in enumerate(caps)]
            middle = R.any_bits(cap1, 3 + accumulate)
            accs = [Acc(cap, fill=f) for cap, f in zip(caps, fills)]
            accs[1].view.view(torch.int32).copy_(torch.from_numpy(middle.view(np.int32)))
            status = torch.full((4,), 7, dtype=torch.uint8, device=_dev())
            norm = Norm(4)
            dg.decompress_data_reduce(ins, [a.view for a in accs], accumulate, None, status, None, dtype=C.DTYPE[ft], scale=THIRD,
                                      out_sumsq=norm.sumsq, out_nonfinite=norm.nonfinite)
            what2 = f"ft={ft} source 1: {what}, accumulate={accumulate}"
            assert status.tolist() == [1, 0, 1, 1], what2
            sumsq, nonfinite = norm.sumsq.tolist(), norm.nonfinite.tolist()
            assert sumsq[1] == 0.0 and nonfinite[1] == 0 and sumsq[2] == 0.0 and nonfinite[2] == 0, (what2, sumsq, nonfinite)
            _same(accs[1].bits(), middle, f"{what2}: the failing member's accumulator")
            for k, i in ((0, 0), (3, 2)):
                with np.errstate(invalid="ignore"):
                    want = scaled(R.reduce_expected(fills[k], [src.wide[s][i] for s in range(3)], bool(accumulate)), THIRD)
                _same(accs[k].bits(), C.bits(want), f"{what2}: neighbour {k}")
                N.check(sumsq[k], nonfinite[k], want, f"{what2}: neighbour {k}")
            assert all(a.guards_intact() for a in accs), what2


# ------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("ft", C.FTS)
def test_the_same_bits_under_every_order_work_list_mode_and_repeat(ft):
    import dietgpu_amd as dg

    L = dg.lib()
    B = 13
    for tile_blocks in C.ORDER_GEOMETRIES:
        tag = f"orders{B}x{tile_blocks}"
        src = R.orders(ft, B, tile_blocks)
        rows, raws = _rows(src, tag, 10), _raws(src, tag)
        members = list(range(B))
        ins = _ins(rows, raws, 2, members, (1,))
        seen = []

        def run(label):
            norm = Norm(B)
            accs, status, _, _ = _call(dg.decompress_data_reduce_mixed, ins, src, members, 1, THIRD, norm)
            assert status.tolist() == [1] * B, label
            seen.append((label, norm.sumsq.cpu().numpy().view(np.uint64).copy(), norm.nonfinite.tolist(), [a.bits() for a in accs]))

        for repeat in range(3):
            run(f"repeat {repeat}")
        for order in (0, 1, 2):
            L.dgpu_debug_set_decoder_order(order)
            try:
                run(f"decoder order {order}")
            finally:
                L.dgpu_debug_set_decoder_order(-1)
        for lists in (1, 0):
            L.dgpu_debug_set_work_lists(lists)
            try:
                run(f"work lists {lists}")
            finally:
                L.dgpu_debug_set_work_lists(-1)
        L.dgpu_debug_set_absent_workgroups(3)
        try:
            run("absent workgroups modulo 3")
        finally:
            L.dgpu_debug_set_absent_workgroups(0)
        want = src.expected(2, True)
        for k in members:
            N.check(float(seen[0][1].view(np.float64)[k]), seen[0][2][k], scaled(want[k], THIRD), f"{tag} ft={ft}: member {k}")
        for label, bits, bad, acc in seen[1:]:
            assert (bits == seen[0][1]).all(), f"{tag} ft={ft}: sumsq under {label} differs in bits from the first call"
            assert bad == seen[0][2], label
            for k in members:
                _same(acc[k], seen[0][3][k], f"{tag} {label}: accumulator {k}")


# ----------------------------------------------------------------------------------------------- routes and batching
def test_routes_agree_and_no_outputs_is_the_call_of_today():
    import dietgpu_amd as dg

    ft, S = C.FTS[1], 3
    src = R.staging(ft)
    rows, raws = _rows(src, "staging", 10), _raws(src, "staging")
    B = len(src.sizes)
    members = list(range(B))
    ins = _ins(rows, raws, S, members, (1,))
    if dg.ops._fast_ops(10) is not None:
        assert hasattr(torch.ops.dietgpu_amd, "decompress_data_reduce_norm")
    got = {}
    try:
        for route in (False, True):
            dg.prefer_torch_ops(route)
            for which in ("both", "sumsq", "nonfinite"):
                norm = Norm(B)
                if which == "sumsq":
                    norm.nonfinite = None
                if which == "nonfinite":
                    norm.sumsq = None
                accs, status, _, used = _call(dg.decompress_data_reduce_mixed, ins, src, members, 1, THIRD, norm)
                assert status.tolist() == [1] * B and used > 0
                got[route, which] = (None if norm.sumsq is None else norm.sumsq.cpu().numpy().view(np.uint64).copy(),
                                     None if norm.nonfinite is None else norm.nonfinite.tolist(), [a.bits() for a in accs])
            accs, status, _, used = _call(dg.decompress_data_reduce_mixed, ins, src, members, 1, THIRD, None)
            assert used == 0  # no temp memory: the scaled call
            for k in members:
                _same(accs[k].bits(), got[route, "both"][2][k], f"torch ops {route}: no outputs, accumulator {k}")
    finally:
        dg.prefer_torch_ops(True)
    ref = got[False, "both"]
    for key, (sumsq, bad, acc) in got.items():
        assert sumsq is None or (sumsq == ref[0]).all(), key
        assert bad is None or bad == ref[1], key
        for k in members:
            _same(acc[k], ref[2][k], f"{key}: accumulator {k}")
    # the C ABI itself, sourceKind NULL, scale 1, and a temp region that is too small: overflow memory, the same result
    flat = [t for member in _ins(rows, raws, S, members, ()) for t in member]
    accs = [Acc(n, fill=src.start[i]) for i, n in enumerate(src.sizes)]
    norm = Norm(B)
    temp = torch.empty(256, dtype=torch.uint8, device=_dev())
    used = ctypes.c_size_t(99)
    rc = dg.lib().dgpu_float_decode_reduce_norm(
        ctypes.c_void_p(temp.data_ptr()), 16, ctypes.byref(used), ft, 10, 1, B, S, (ctypes.c_void_p * (B * S))(*[r.data_ptr() for r in flat]),
        (ctypes.c_uint32 * (B * S))(*[r.numel() for r in flat]), None, 1.0, (ctypes.c_void_p * B)(*[a.view.data_ptr() for a in accs]),
        (ctypes.c_uint32 * B)(*src.sizes), None, None, ctypes.c_void_p(norm.sumsq.data_ptr()), ctypes.c_void_p(norm.nonfinite.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, dg.lib().dgpu_last_error()
    assert 16 < used.value <= dg.lib().dgpu_float_reduce_norm_temp_bytes(ft, B, max(src.sizes), 0)
    want = src.expected(S, True)
    for k in members:
        _same(accs[k].bits(), C.bits(want[k]), f"C ABI: accumulator {k}")
        N.check(norm.sumsq[k].item(), norm.nonfinite[k].item(), want[k], f"C ABI, scale 1: member {k}")


def test_a_lone_signalling_nan_keeps_its_bits_with_scale_one():
    import dietgpu_amd as dg

    for ft in C.FTS:
        n = 2 * C.BLK + 777
        w = R.any_bits(n, 300)
        w = w if ft == O.FLOAT32 else (w >> 16).astype(np.uint16)
        w[5] = C.EXP_MASK[ft] | 1
        archive = _upload(O.float_compress(ft, w, 10))
        plain, a = Acc(n), Acc(n)
        norm = Norm(1)
        dg.decompress_data_accumulate([archive], [plain.view], False, None, None, None, dtype=C.DTYPE[ft])
        dg.decompress_data_reduce([[archive]], [a.view], False, None, None, None, dtype=C.DTYPE[ft], out_sumsq=norm.sumsq, out_nonfinite=norm.nonfinite)
        _same(a.bits(), plain.bits(), f"ft={ft}: against decompress_data_accumulate")
        N.check(norm.sumsq.item(), norm.nonfinite.item(), plain.bits().view(np.float32), f"ft={ft} any bits")


def test_more_than_64_members():
    import dietgpu_amd as dg

    ft, B = O.BFLOAT16, 67
    src = R.orders(ft, B, 4)
    tag = f"orders{B}x4"
    _check_case(src, tag, 2, 1, THIRD)


# -------------------------------------------------------------------------------------------------------------- graph
def test_graph_replay_measures_the_changed_sources():
    """a warm call, the same call captured, replays after the raw source's words were changed in place: the accumulators
    and both outputs follow"""
    import dietgpu_amd as dg

    ft, S, members = C.FTS[1], 3, [0, 1, 5]
    src = R.staging(ft)
    rows = _rows(src, "staging", 10)
    raw = [_raw(ft, src.words[1][i]) for i in members]  # (private copies: they are overwritten below)
    ins = [[rows[0][i], raw[k], rows[2][i]] for k, i in enumerate(members)]
    accs = [Acc(src.sizes[i]) for i in members]
    views = [a.view for a in accs]
    status = torch.zeros(len(members), dtype=torch.uint8, device=_dev())
    norm = Norm(len(members))

    def call():  # (dtype given: nothing synchronises)
        dg.decompress_data_reduce_mixed(ins, views, False, None, status, None, dtype=C.DTYPE[ft], scale=THIRD, out_sumsq=norm.sumsq,
                                        out_nonfinite=norm.nonfinite)

    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call()  # the warm call: makes the parameter block resident and the overflow memory large enough
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            call()
        torch.cuda.synchronize()
        for replay, middle in enumerate((1, 3)):  # the middle source: its own words, then those of source 3
            for k, i in enumerate(members):
                raw[k].copy_(torch.from_numpy(src.words[middle][i].view(C.SIGNED[ft]).copy()).view(C.DTYPE[ft]))
            for a in accs:
                a.view.fill_(float("nan"))
            status.fill_(7)
            norm.sumsq.fill_(-1.0)
            norm.nonfinite.fill_(-7)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert status.tolist() == [1] * len(members)
            for k, i in enumerate(members):
                want = scaled(R.reduce_expected(None, [src.wide[0][i], src.wide[middle][i], src.wide[2][i]], False), THIRD)
                _same(accs[k].bits(), C.bits(want), f"replay {replay}: member {i}")
                N.check(norm.sumsq[k].item(), norm.nonfinite[k].item(), want, f"replay {replay}: member {i}")
                assert accs[k].guards_intact()
        del graph
    finally:
        dg.lib().dgpu_release_graph_state()
