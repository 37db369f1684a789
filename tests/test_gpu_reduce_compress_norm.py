"""The norm outputs of reduce-compress on the GPU (dgpu_float_reduce_compress_norm, k_ans_decode_reduce_mixed_stats_norm):
per member, out_sumsq = the sum of squares (float64) of the finite words of the ARCHIVE -- the float32 sums, scaled,
rounded to the archive type as the cast encoder rounds them (tests/cast_ref.py) -- and out_nonfinite = the number of its
words that are inf or NaN.  This is the tensor every rank holds after the all-gather: a float32 sum of 70000 is finite,
its float16 rounding is not.

Expected values come from tests/norm_ref.py (math.fsum of exact float64 squares; the bound of n * 2**-52 is the
kernel's alone).  Accumulators, status, sizes, archives and archive sizes must be, bit for bit, those of the same call
without the two outputs."""
import ctypes

import numpy as np
import pytest
import torch

import accum_cases as C
import cast_ref
import norm_ref as N
import oracle as O
import reduce_cases as R
from test_gpu_accumulate import Acc, _dev
from test_gpu_reduce import _gpu
from test_gpu_reduce_compress import FTS, Out, _rows, _same, _upload
from test_gpu_reduce_mixed import _ins, _raw, _raws
from test_gpu_reduce_norm import THIRD, Norm, _denormal_words, _planted, _same_words, scaled

pytestmark = pytest.mark.gpu


def archive_words(ft, words):
    """float32 words -> the words of the archive a cast of them holds, widened to float32"""
    return C.widen(ft, cast_ref.cast_ref(C.bits(words), ft))


def _call(ft, ins, accs, accumulate, scale, norm, prob_bits=10, temp=None):
    import dietgpu_amd as dg

    mixed = any(t.dtype != torch.uint8 for member in ins for t in member)
    f = dg.decompress_data_reduce_compress_mixed if mixed else dg.decompress_data_reduce_compress
    out = Out(ft, [a.n for a in accs])
    kw = {} if norm is None else {"out_sumsq": norm.sumsq, "out_nonfinite": norm.nonfinite}
    comp, csizes, used = f(ins, [a.view for a in accs], accumulate, temp, out.status, out.sizes, out.comp, out.csizes, prob_bits=prob_bits,
                           dtype=C.DTYPE[ft], scale=scale, **kw)
    assert comp.data_ptr() == out.comp.data_ptr() and csizes.data_ptr() == out.csizes.data_ptr()
    return out, used


def _check_case(src, tag, S, accumulate, scale, raw_at=(), offsets=None, prob_bits=10):
    import dietgpu_amd as dg

    ft = src.ft
    rows, raws = _rows(src, tag, prob_bits), _raws(src, tag)
    members = list(range(len(src.sizes)))
    B = len(members)
    ins = _ins(rows, raws, S, members, raw_at)

    def fresh():
        return [Acc(src.sizes[i], offsets[k] if offsets else 0, fill=src.start[i] if accumulate else None) for k, i in enumerate(members)]

    norm = Norm(B)
    accs, plain = fresh(), fresh()
    out, used = _call(ft, ins, accs, accumulate, scale, norm, prob_bits)
    out0, used0 = _call(ft, ins, plain, accumulate, scale, None, prob_bits)
    what = f"{tag} ft={ft} S={S} accumulate={accumulate} scale={scale} raw at {list(raw_at)}"
    assert used0 < used <= dg.lib().dgpu_float_reduce_norm_temp_bytes(ft, B, max(src.sizes), 1), (what, used0, used)
    assert out.status.tolist() == out0.status.tolist() == [1] * B, what
    assert out.sizes.tolist() == out0.sizes.tolist() == list(src.sizes), what
    arch, arch0 = out.archives(), out0.archives()
    want = src.expected(S, bool(accumulate))
    sumsq, nonfinite = norm.sumsq.tolist(), norm.nonfinite.tolist()
    for k in members:
        words = scaled(want[k], scale)
        _same(accs[k].bits(), plain[k].bits(), f"{what}: accumulator {k} against the call without the outputs")
        _same_words(accs[k].bits(), C.bits(words), f"{what}: accumulator {k} against the host")
        assert accs[k].guards_intact(), what
        _same(arch[k], arch0[k], f"{what}: archive {k} against the call without the outputs")
        N.check(sumsq[k], nonfinite[k], archive_words(ft, words), f"{what}: member {k}")


# ------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("scale", [None, THIRD])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("ft", FTS)
def test_values_on_the_staging_and_partial_block_cases(ft, S, accumulate, scale):
    _check_case(R.staging(ft), "staging", S, accumulate, scale)
    if S <= 2:
        for lead in (0, 3):
            src = R.tails(ft, lead)
            _check_case(src, f"tails{lead}", S, accumulate, scale, offsets=[i % 4 for i in range(len(src.sizes))])


@pytest.mark.parametrize("ft", FTS)
def test_a_raw_row_as_the_last_and_as_the_first_source(ft):
    for raw_at in ((2,), (0,)):
        for accumulate, scale in ((0, THIRD), (1, None)):
            _check_case(R.staging(ft), "staging", 3, accumulate, scale, raw_at=raw_at)


def test_table_precision_eleven():
    _check_case(R.staging(O.FLOAT16), "staging", 2, 1, THIRD, prob_bits=11)


# ----------------------------------------------------------------------------------------------------- planted words
@pytest.mark.parametrize("ft", FTS)
def test_planted_words(ft):
    """as in test_gpu_reduce_norm.py, measured behind the rounding: the two words near the largest finite float32 round to
    bfloat16 words whose squares still overflow float32 (float16: to infinities, which are counted); float16: the sum
    40000 + 30000 is +inf in the archive -- counted, and left out of the squared norm"""
    w, start, pos = _planted(ft)
    n = w[0].size
    archives = [_upload(O.float_compress(ft, x, 10)) for x in w]
    raws = [_raw(ft, x) for x in w]
    wide = [C.widen(ft, x) for x in w]
    with np.errstate(invalid="ignore", over="ignore"):
        want = R.reduce_expected(start, wide, True)
    measured = archive_words(ft, want)
    exact, bad, _ = N.stats(measured)
    if ft == O.FLOAT16:
        assert want[pos["sum"]] == np.float32(70000.0) and np.isposinf(measured[pos["sum"]])
        assert bad == 3 + 2 + 1  # the planted three, the two large words and the sum
    else:
        assert bad == 3 and exact > 1.9e77
        with np.errstate(over="ignore"):
            assert np.isinf(np.sum(np.square(measured[np.isfinite(measured)], dtype=np.float32), dtype=np.float32))
    for ins in ([archives[0], archives[1]], [archives[0], raws[1]]):
        a = Acc(n, fill=start)
        norm = Norm(1)
        out, _ = _call(ft, [ins], [a], True, None, norm)
        assert out.status.tolist() == [1]
        _same_words(a.bits(), C.bits(want), f"ft={ft}: the accumulator")
        N.check(norm.sumsq.item(), norm.nonfinite.item(), measured, f"ft={ft} planted words")


@pytest.mark.parametrize("ft", FTS)
def test_denormals_are_finite_words_and_their_squares_are_summed(ft):
    """a member that holds nothing but zeros and denormals, which the rounding to the archive type keeps: a kernel that
    flushed them would report 0.0"""
    w = _denormal_words(ft)
    n = w.size
    zeros = np.zeros(n, np.uint16)
    wide = C.widen(ft, w)
    measured = archive_words(ft, wide)
    want_sq, bad, _ = N.stats(measured)
    assert bad == 0 and 0.0 < want_sq < 1e-6 and np.array_equal(C.bits(measured), C.bits(wide))
    sources = {"archive": _upload(O.float_compress(ft, w, 10)), "raw": _raw(ft, w)}
    others = {"archive": _upload(O.float_compress(ft, zeros, 10)), "raw": _raw(ft, zeros)}
    for ins in (["archive"], ["raw"], ["archive", "raw"], ["raw", "archive"]):
        for accumulate in (0, 1):
            a = Acc(n, fill=np.zeros(n, np.float32))
            norm = Norm(1)
            out, _ = _call(ft, [[sources[ins[0]]] + [others[k] for k in ins[1:]]], [a], accumulate, None, norm)
            assert out.status.tolist() == [1]
            _same(a.bits(), C.bits(wide), f"ft={ft} {ins} accumulate={accumulate}: the accumulator")
            _same(out.archives()[0], O.float_compress(ft, w, 10), f"ft={ft} {ins} accumulate={accumulate}: the archive")
            N.check(norm.sumsq.item(), norm.nonfinite.item(), measured, f"ft={ft} {ins} accumulate={accumulate} denormals")


# ------------------------------------------------------------------------------------------------- a factor of one
@pytest.mark.parametrize("ft", FTS)
def test_without_a_scale_any_bit_pattern_is_stored_as_the_unscaled_call_stores_it(ft):
    """the counting sink of the norm form multiplies by a factor other than 1 only: with scale None (and 1.0) the
    accumulators, NaN payloads and a lone signalling NaN included, and the archives are bit for bit those of the unscaled
    call without the outputs"""
    n = 2 * C.BLK + 777
    exp = C.EXP_MASK[ft]
    words = []
    for s in range(2):
        w = (R.any_bits(n, 400 + s) >> 16).astype(np.uint16)
        w[5 + s] = exp | 1  # a signalling NaN of the type
        w[C.BLK + 9] = exp  # +inf
        words.append(w)
    assert all((((w & 0x7FFF) > exp).sum() > 10) for w in words)
    archives = [_upload(O.float_compress(ft, w, 10)) for w in words]
    raws = [_raw(ft, w) for w in words]
    start = R.any_bits(n, 410).view(np.float32)
    for ins in ([archives[0]], [raws[0]], [archives[0], raws[1]], [raws[0], archives[1]]):
        for accumulate in (0, 1):
            plain = Acc(n, fill=start)
            out0, _ = _call(ft, [ins], [plain], accumulate, None, None)
            assert out0.status.tolist() == [1]
            for scale in (None, 1.0):
                a = Acc(n, fill=start)
                norm = Norm(1)
                out, _ = _call(ft, [ins], [a], accumulate, scale, norm)
                what = f"ft={ft} S={len(ins)} raw {[t.dtype != torch.uint8 for t in ins]} accumulate={accumulate} scale={scale}"
                assert out.status.tolist() == [1], what
                _same(a.bits(), plain.bits(), what + ": the accumulator against the unscaled call")
                _same(out.archives()[0], out0.archives()[0], what + ": the archive against the unscaled call")
                assert a.guards_intact(), what
                N.check(norm.sumsq.item(), norm.nonfinite.item(), archive_words(ft, plain.bits().view(np.float32)), what)
            if len(ins) == 1 and not accumulate and ft == O.BFLOAT16:  # widening is a shift: the signalling NaN keeps its bits
                _same(plain.bits(), words[0].astype(np.uint32) << 16, "bfloat16 words are stored shifted")


# --------------------------------------------------------------------------------------------- failed and empty members
@pytest.mark.parametrize("ft", FTS)
def test_a_failed_member_and_an_empty_member_get_zeros(ft):
    name = "two 4-block tiles"
    tile_blocks, sizes, cap1 = C.MALFORMED_BATCHES[name]
    src = R.malformed(ft, name)
    rows = _rows(src, "malformed " + name, 10)
    good = src.archives(10)[1][1]
    corruptions = list(C.corruptions(ft, good, sizes[1], tile_blocks))
    empty = _gpu(("empty", ft), lambda: _upload(O.float_compress(ft, np.zeros(0, np.uint16), 10)))
    what, bad = corruptions[0]
    for accumulate in (0, 1):
        # (reduce-compress: every source states exactly the capacity, so the failing member is as large as its sources say)
        ins = [[rows[s][0] for s in range(3)], [rows[0][1], _upload(bad), rows[2][1]], [empty] * 3, [rows[s][2] for s in range(3)]]
        caps = [sizes[0], sizes[1], 0, sizes[2]]
        fills = [R.finite_bits(cap, 10 * k + accumulate) for k, cap in enumerate(caps)]
        middle = R.any_bits(sizes[1], 3 + accumulate)
        accs = [Acc(cap, fill=f) for cap, f in zip(caps, fills)]
        accs[1].view.view(torch.int32).copy_(torch.from_numpy(middle.view(np.int32)))
        norm = Norm(4)
        out, _ = _call(ft, ins, accs, accumulate, THIRD, norm)
        what2 = f"ft={ft} source 1: {what}, accumulate={accumulate}"
        assert out.status.tolist() == [1, 0, 1, 1], what2
        sumsq, nonfinite = norm.sumsq.tolist(), norm.nonfinite.tolist()
        assert sumsq[1] == 0.0 and nonfinite[1] == 0 and sumsq[2] == 0.0 and nonfinite[2] == 0, (what2, sumsq, nonfinite)
        _same(accs[1].bits(), middle, f"{what2}: the failing member's accumulator")
        for k, i in ((0, 0), (3, 2)):
            with np.errstate(invalid="ignore"):
                want = scaled(R.reduce_expected(fills[k], [src.wide[s][i] for s in range(3)], bool(accumulate)), THIRD)
            _same(accs[k].bits(), C.bits(want), f"{what2}: neighbour {k}")
            N.check(sumsq[k], nonfinite[k], archive_words(ft, want), f"{what2}: neighbour {k}")
        assert all(a.guards_intact() for a in accs), what2


# ------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("ft", FTS)
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
            accs = [Acc(src.sizes[i], fill=src.start[i]) for i in members]
            out, _ = _call(ft, ins, accs, 1, THIRD, norm)
            assert out.status.tolist() == [1] * B, label
            seen.append((label, norm.sumsq.cpu().numpy().view(np.uint64).copy(), norm.nonfinite.tolist(), out.archives()))

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
            N.check(float(seen[0][1].view(np.float64)[k]), seen[0][2][k], archive_words(ft, scaled(want[k], THIRD)), f"{tag} ft={ft}: member {k}")
        for label, bits, bad, arch in seen[1:]:
            assert (bits == seen[0][1]).all(), f"{tag} ft={ft}: sumsq under {label} differs in bits from the first call"
            assert bad == seen[0][2], label
            for k in members:
                _same(arch[k], seen[0][3][k], f"{tag} {label}: archive {k}")


# ----------------------------------------------------------------------------------------------- routes and batching
def test_routes_agree_and_no_outputs_is_the_call_of_today():
    import dietgpu_amd as dg

    ft, S = O.BFLOAT16, 3
    src = R.staging(ft)
    rows, raws = _rows(src, "staging", 10), _raws(src, "staging")
    B = len(src.sizes)
    members = list(range(B))
    ins = _ins(rows, raws, S, members, (1,))
    if dg.ops._fast_ops(10) is not None:
        assert hasattr(torch.ops.dietgpu_amd, "decompress_data_reduce_compress_norm")
    need = dg.lib().dgpu_float_reduce_norm_temp_bytes(ft, B, max(src.sizes), 1)
    got = {}
    try:
        for route in (False, True):
            dg.prefer_torch_ops(route)
            for temp in (None, torch.empty(need, dtype=torch.uint8, device=_dev()), torch.empty(1024, dtype=torch.uint8, device=_dev())):
                accs = [Acc(n, fill=src.start[i]) for i, n in enumerate(src.sizes)]
                norm = Norm(B)
                out, used = _call(ft, ins, accs, 1, THIRD, norm, temp=temp)
                assert out.status.tolist() == [1] * B and 0 < used <= need
                got[route, None if temp is None else temp.numel()] = (norm.sumsq.cpu().numpy().view(np.uint64).copy(), norm.nonfinite.tolist(),
                                                                     [a.bits() for a in accs], out.archives())
            accs = [Acc(n, fill=src.start[i]) for i, n in enumerate(src.sizes)]
            out, used = _call(ft, ins, accs, 1, THIRD, None)
            assert used <= dg.lib().dgpu_float_reduce_compress_temp_bytes(ft, B, max(src.sizes))
            for k in members:
                _same(accs[k].bits(), got[route, None][2][k], f"torch ops {route}: no outputs, accumulator {k}")
                _same(out.archives()[k], got[route, None][3][k], f"torch ops {route}: no outputs, archive {k}")
    finally:
        dg.prefer_torch_ops(True)
    ref = got[False, None]
    for key, (sumsq, bad, acc, arch) in got.items():
        assert (sumsq == ref[0]).all() and bad == ref[1], key
        for k in members:
            _same(acc[k], ref[2][k], f"{key}: accumulator {k}")
            _same(arch[k], ref[3][k], f"{key}: archive {k}")


@pytest.mark.parametrize("ft", FTS)
def test_more_than_64_members_counts_in_temp_memory(ft):
    _check_case(R.orders(ft, 67, 4), "orders67x4", 2, 1, THIRD, raw_at=(1,))


# -------------------------------------------------------------------------------------------------------------- graph
def test_graph_replay_measures_the_changed_sources():
    import dietgpu_amd as dg

    ft, S, members = O.BFLOAT16, 3, [0, 1, 5]
    src = R.staging(ft)
    rows = _rows(src, "staging", 10)
    raw = [_raw(ft, src.words[1][i]) for i in members]  # (private copies: they are overwritten below)
    ins = [[rows[0][i], raw[k], rows[2][i]] for k, i in enumerate(members)]
    accs = [Acc(src.sizes[i]) for i in members]
    out = Out(ft, [a.n for a in accs])
    norm = Norm(len(members))
    temp = torch.empty(dg.lib().dgpu_float_reduce_norm_temp_bytes(ft, len(members), max(a.n for a in accs), 1), dtype=torch.uint8, device=_dev())

    def call():  # (dtype given: nothing synchronises)
        dg.decompress_data_reduce_compress_mixed(ins, [a.view for a in accs], False, temp, out.status, out.sizes, out.comp, out.csizes,
                                                 dtype=C.DTYPE[ft], scale=THIRD, out_sumsq=norm.sumsq, out_nonfinite=norm.nonfinite)

    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call()  # the warm call: makes the parameter blocks resident
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            call()
        torch.cuda.synchronize()
        for replay, middle in enumerate((1, 3)):
            for k, i in enumerate(members):
                raw[k].copy_(torch.from_numpy(src.words[middle][i].view(C.SIGNED[ft]).copy()).view(C.DTYPE[ft]))
            for a in accs:
                a.view.fill_(float("nan"))
            out.status.fill_(7)
            norm.sumsq.fill_(-1.0)
            norm.nonfinite.fill_(-7)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert out.status.tolist() == [1] * len(members)
            arch = out.archives()
            for k, i in enumerate(members):
                want = scaled(R.reduce_expected(None, [src.wide[0][i], src.wide[middle][i], src.wide[2][i]], False), THIRD)
                _same(accs[k].bits(), C.bits(want), f"replay {replay}: member {i}")
                _same(arch[k], O.float_compress(ft, cast_ref.cast_ref(C.bits(want), ft), 10), f"replay {replay}: archive of member {i}")
                N.check(norm.sumsq[k].item(), norm.nonfinite[k].item(), archive_words(ft, want), f"replay {replay}: member {i}")
        del graph
    finally:
        dg.lib().dgpu_release_graph_state()
