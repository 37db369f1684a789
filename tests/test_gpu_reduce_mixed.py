"""Decode-reduce with mixed sources on the GPU (dgpu_float_decode_reduce_mixed, k_ans_decode_reduce_mixed): a source of
a sum is an archive or a RAW row of float words, added in its place in source order.

The specification is an equivalence: the call leaves, bit for bit, what dgpu_float_decode_reduce leaves when every raw
row is replaced by its archive.  So the inputs and expected values are those of tests/reduce_cases.py unchanged -- a raw
source is `Sources.words[s][i]` uploaded instead of `Sources.archives(P)[s][i]` -- and every comparison is on uint32
views, every word of it."""
import ctypes

import numpy as np
import pytest
import torch

import accum_cases as C
import oracle as O
import reduce_cases as R
from test_gpu_accumulate import Acc, _dev
from test_gpu_reduce import _gpu, _rows, _same, _upload

pytestmark = pytest.mark.gpu


def _raw(ft, words, offset=0, extra=0):
    """`words` (numpy, the type's word) as a 1-D tensor of the float dtype that starts `offset` words past a 16-byte
    boundary, with `extra` more words of the buffer behind it in the view"""
    n = words.size
    buf = torch.zeros(offset + n + extra + 8, dtype=C.DTYPE[ft], device=_dev())
    assert buf.data_ptr() % 16 == 0
    view = buf[offset : offset + n + extra]
    view[:n].copy_(torch.from_numpy(words.view(C.SIGNED[ft]).copy()).view(C.DTYPE[ft]))
    return view


def _raws(src, tag):
    """[source][element] raw rows of `src` on the GPU (16-byte aligned), uploaded once"""
    return _gpu((tag, src.ft, "raw"), lambda: [[_raw(src.ft, w) for w in row] for row in src.words])


def patterns(S):
    """the raw positions the issue names: none, first only, last only, one in the middle, alternating, all"""
    named = [("none", ()), ("first", (0,)), ("last", (S - 1,)), ("middle", (S // 2,)), ("alternating", tuple(range(0, S, 2))),
             ("all", tuple(range(S)))]
    seen, out = set(), []
    for name, p in named:
        if p not in seen:
            seen.add(p)
            out.append((name, p))
    return out


def _ins(rows, raws, S, members, raw_at):
    return [[raws[s][i] if s in raw_at else rows[s][i] for s in range(S)] for i in members]


def _mixed_and_check(src, rows, raws, S, prob_bits, members, accumulate, raw_at, what, offsets=None, plain=False):
    """one mixed call for `members` with the first S sources, those at `raw_at` raw: status, sizes, every accumulator
    word, the guards; with `plain`, the all-archive call on fresh accumulators must leave the same"""
    import dietgpu_amd as dg

    B = len(members)

    def fresh():
        return [Acc(src.sizes[i], offsets[k] if offsets else 0, fill=src.start[i] if accumulate else None) for k, i in enumerate(members)]

    accs = fresh()
    status = torch.full((B,), 7, dtype=torch.uint8, device=_dev())
    sizes = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    used = dg.decompress_data_reduce_mixed(_ins(rows, raws, S, members, raw_at), [a.view for a in accs], accumulate, None, status, sizes,
                                           prob_bits=prob_bits, dtype=C.DTYPE[src.ft])
    what = f"ft={src.ft} probBits={prob_bits} S={S} accumulate={accumulate} raw at {list(raw_at)} {what}"
    assert used == 0, what
    assert status.tolist() == [1] * B, what
    assert sizes.tolist() == [src.sizes[i] for i in members], what
    want = src.expected(S, bool(accumulate))
    got = [a.bits() for a in accs]
    for k, i in enumerate(members):
        _same(got[k], C.bits(want[i]), f"{what}: member {k} ({src.sizes[i]} words)")
        assert accs[k].guards_intact(), f"{what}: member {k}: guard words overwritten"
    if plain:
        ref = fresh()
        st = torch.zeros(B, dtype=torch.uint8, device=_dev())
        sz = torch.zeros(B, dtype=torch.int32, device=_dev())
        dg.decompress_data_reduce(_ins(rows, raws, S, members, ()), [a.view for a in ref], accumulate, None, st, sz, prob_bits=prob_bits,
                                  dtype=C.DTYPE[src.ft])
        assert st.tolist() == status.tolist() and sz.tolist() == sizes.tolist(), what
        for k, a in enumerate(ref):
            _same(got[k], a.bits(), f"{what}: member {k} against dgpu_float_decode_reduce")


# ------------------------------------------------------------------------------------------------------ equivalence
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("prob_bits", C.PROB_BITS)
@pytest.mark.parametrize("ft", C.FTS)
def test_mixed_equals_the_sequence(ft, prob_bits, S, accumulate):
    """the staging shapes (16- and 4-block tiles, whole, ring, mixed and boundary waves, partial last blocks) with every
    raw pattern: archive after raw and raw after archive, raw first (stored), raw last, all raw"""
    src = R.staging(ft)
    rows, raws = _rows(src, "staging", prob_bits), _raws(src, "staging")
    members = list(range(len(src.sizes)))
    for name, raw_at in patterns(S):
        _mixed_and_check(src, rows, raws, S, prob_bits, members, accumulate, raw_at, f"staging shapes, pattern {name}", plain=name == "none")


# -------------------------------------------------------------------------------------------------- any bit pattern
@pytest.mark.parametrize("ft", C.FTS)
def test_any_bit_pattern_adds_like_its_archive(ft):
    """rows of random bits -- NaN payloads, infinities, denormals -- raw and as archives: GPU against GPU, so whatever
    the adder does with a NaN's payload it does in both"""
    import dietgpu_amd as dg

    n, S = 2 * C.BLK + 777, 3
    words = []
    for s in range(S):
        w = R.any_bits(n, 100 + s)
        w = w if ft == O.FLOAT32 else (w >> 16).astype(np.uint16)
        # (random 16-bit words need not hold an infinity: +inf, -inf, the smallest denormal and a NaN with a payload are
        # planted, rotated from source to source so that inf meets -inf and NaN meets inf)
        exp, low = C.EXP_MASK[ft], C.EXP_LOW[ft]
        specials = [exp, exp | (exp + low), 1, exp | 5]
        for k in range(len(specials)):
            w[C.BLK - 2 + k] = specials[(k + s) % len(specials)]
        words.append(w)
    wide = C.widen(ft, words[1])
    assert np.isnan(wide).any() and np.isposinf(wide).any() and np.isneginf(wide).any()
    assert ((words[1] & exp) == 0).any()  # denormals of the type
    archives = [_upload(O.float_compress(ft, w, 10)) for w in words]
    raws = [_raw(ft, w) for w in words]
    start = R.any_bits(n, 200)
    for accumulate in (0, 1):
        def run(f, ins):
            a = Acc(n)
            a.view.view(torch.int32).copy_(torch.from_numpy(start.view(np.int32)))
            status = torch.zeros(1, dtype=torch.uint8, device=_dev())
            f([ins], [a.view], accumulate, None, status, None, dtype=C.DTYPE[ft])
            assert status.tolist() == [1]
            assert a.guards_intact()
            return a.bits()

        want = run(dg.decompress_data_reduce, archives)
        for raw_at in ((0,), (1,), (2,), (0, 2), (0, 1, 2)):
            got = run(dg.decompress_data_reduce_mixed, [raws[s] if s in raw_at else archives[s] for s in range(S)])
            _same(got, want, f"ft={ft} accumulate={accumulate} raw at {list(raw_at)}")


# ------------------------------------------------------------------------------------------------------------ order
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("ft", C.FTS)
def test_a_raw_source_is_added_in_its_place(ft, accumulate):
    import dietgpu_amd as dg

    hi, lo, tiny = R.ORDER_VALUES
    n = R.ORDER_WORDS
    arch = {v: _gpu(("order", ft, v), lambda v=v: _upload(O.float_compress(ft, R.constant_words(ft, v), 10))) for v in R.ORDER_VALUES}
    raw = {v: _raw(ft, R.constant_words(ft, v)) for v in R.ORDER_VALUES}
    for order, total in (((hi, lo, tiny), 2.0 ** -10), ((tiny, hi, lo), 0.0)):
        for raw_pos in range(3):
            start = np.zeros(n, np.float32)
            a = Acc(n, fill=start if accumulate else None)
            status = torch.zeros(1, dtype=torch.uint8, device=_dev())
            ins = [raw[v] if k == raw_pos else arch[v] for k, v in enumerate(order)]
            dg.decompress_data_reduce_mixed([ins], [a.view], accumulate, None, status, None, dtype=C.DTYPE[ft])
            assert status.tolist() == [1]
            want = R.reduce_expected(start, [np.full(n, v, np.float32) for v in order], bool(accumulate))
            assert (want == np.float32(total)).all()
            _same(a.bits(), C.bits(want), f"ft={ft} accumulate={accumulate} sources {order}, raw at {raw_pos}")
            assert a.guards_intact()


# ------------------------------------------------------------------------------------------------------------ tails
@pytest.mark.parametrize("lead", [0, 3])
@pytest.mark.parametrize("ft", C.FTS)
def test_partial_last_blocks(ft, lead):
    """every length of a last block; with lead 0 the elements are single partial blocks on the 4-block tiles, where all
    half-waves but one have no block"""
    src = R.tails(ft, lead)
    rows, raws = _rows(src, f"tails{lead}", 10), _raws(src, f"tails{lead}")
    members = list(range(len(src.sizes)))
    for accumulate in (0, 1):
        for raw_at in ((0,), (1,)):
            _mixed_and_check(src, rows, raws, 2, 10, members, accumulate, raw_at, f"lead {lead}", offsets=[i % 4 for i in members])


# --------------------------------------------------------------------------------------------------- base alignment
@pytest.mark.parametrize("offset", [1, 2, 3, 8])
@pytest.mark.parametrize("ft", C.FTS)
def test_raw_rows_of_any_word_alignment(ft, offset):
    """rows that start 1, 3 and 8 words into a 16-byte aligned buffer (2 too: the 4-byte base of a 16-bit row), so the
    kernel takes its 2-byte, 4-byte and 16-byte loads; accumulators 1 to 3 words off as well"""
    src = R.staging(ft)
    rows = _rows(src, "staging", 10)
    raws = _gpu(("staging", ft, "raw", offset), lambda: [[_raw(ft, w, offset) for w in row] for row in src.words[:2]])
    word = 2 if ft != O.FLOAT32 else 4
    assert raws[0][0].data_ptr() % 16 == (offset * word) % 16
    members = list(range(len(src.sizes)))
    for accumulate in (0, 1):
        for raw_at in ((0,), (1,), (0, 1)):
            _mixed_and_check(src, rows, raws, 2, 10, members, accumulate, raw_at, f"row offset {offset} words",
                             offsets=[1 + (i + offset) % 3 for i in members])


# -------------------------------------------------------------------------------------------- geometry and work lists
@pytest.mark.parametrize("B", [13, 67])
@pytest.mark.parametrize("ft", C.FTS)
def test_workgroup_orders_and_work_lists(ft, B):
    import dietgpu_amd as dg

    L = dg.lib()
    for tile_blocks in C.ORDER_GEOMETRIES:
        src = R.orders(ft, B, tile_blocks)
        rows, raws = _rows(src, f"orders{B}x{tile_blocks}", 10), _raws(src, f"orders{B}x{tile_blocks}")
        members = list(range(B))
        assert -(-max(src.sizes) // C.BLK) == C.ORDER_GEOMETRIES[tile_blocks][1]  # this geometry, two tiles per member
        for order, raw_at in ((0, (0,)), (1, (1,)), (2, (0,))):
            L.dgpu_debug_set_decoder_order(order)
            try:
                _mixed_and_check(src, rows, raws, 2, 10, members, order % 2, raw_at, f"order {order}, {tile_blocks}-block tiles")
            finally:
                L.dgpu_debug_set_decoder_order(-1)
        for lists in (1, 0):
            L.dgpu_debug_set_work_lists(lists)
            try:
                for accumulate, raw_at in ((0, (1,)), (1, (0,)), (0, (0, 1))):
                    _mixed_and_check(src, rows, raws, 2, 10, members, accumulate, raw_at, f"work lists {lists}, {tile_blocks}-block tiles")
            finally:
                L.dgpu_debug_set_work_lists(-1)


# --------------------------------------------------------------------------------------------------- all or nothing
def _failure_cases(ft, name, src, rows, raws):
    """-> [(what, the middle member's sources, its capacity, the size reported)]"""
    tile_blocks, sizes, cap1 = C.MALFORMED_BATCHES[name]
    n1 = sizes[1]
    arch = [rows[s][1] for s in range(3)]
    raw = [raws[s][1] for s in range(3)]
    longer = [_raw(ft, src.words[s][1], extra=1) for s in range(3)]
    out = []
    for s in range(3):
        ins = [arch[0], arch[1], arch[2]]
        ins[s] = longer[s]
        out.append((f"raw source {s} states one word more", ins, cap1, n1 + 1 if s == 0 else n1))
        ins = [raw[0], raw[1], raw[2]]
        ins[s] = raw[s][: n1 - 1]
        # (source 0 states its own count; a later source of another count leaves source 0's)
        out.append((f"raw source {s} states one word fewer, raw siblings", ins, cap1, n1 - 1 if s == 0 else n1))
        ins = [arch[0], arch[1], arch[2]]
        ins[s] = raw[s]
        out.append((f"raw source {s} longer than the capacity", ins, n1 - 1, n1))
    out.append(("all raw, longer than the capacity", raw, n1 - 1, n1))
    good = src.archives(10)[1][1]
    for what, bad in C.corruptions(ft, good, n1, tile_blocks):
        out.append((f"archive source 1 among raw siblings: {what}", [raw[0], _upload(bad), raw[2]], cap1, n1))
    out.append(("archive source 1 among raw siblings: truncated by 16 bytes", [raw[0], arch[1][: arch[1].numel() - 16], raw[2]], cap1, n1))
    return out


@pytest.mark.parametrize("name", list(C.MALFORMED_BATCHES))
@pytest.mark.parametrize("ft", C.FTS)
def test_a_member_with_one_bad_source_keeps_every_bit(ft, name):
    """three members, three sources each; the middle member has a raw source whose count disagrees, or that is longer
    than the capacity, or a malformed archive among raw siblings: status [1, 0, 1], the middle accumulator as it was
    (any bits), the neighbours -- themselves mixed -- summed"""
    import dietgpu_amd as dg

    _, sizes, _ = C.MALFORMED_BATCHES[name]
    src = R.malformed(ft, name)
    rows, raws = _rows(src, "malformed " + name, 10), _raws(src, "malformed " + name)
    for what, middle_ins, cap1, reported in _failure_cases(ft, name, src, rows, raws):
        ins = [[raws[0][0], rows[1][0], rows[2][0]], middle_ins, [rows[0][2], rows[1][2], raws[2][2]]]
        caps = [sizes[0], cap1, sizes[2]]
        for accumulate in (0, 1):
            fills = [R.finite_bits(cap, 10 * k + accumulate) for k, cap in enumerate(caps)]
            middle = R.any_bits(cap1, 3 + accumulate)
            assert np.isnan(middle.view(np.float32)).any()
            accs = [Acc(cap, fill=f) for cap, f in zip(caps, fills)]
            accs[1].view.view(torch.int32).copy_(torch.from_numpy(middle.view(np.int32)))
            status = torch.full((3,), 7, dtype=torch.uint8, device=_dev())
            out_sizes = torch.full((3,), -7, dtype=torch.int32, device=_dev())
            dg.decompress_data_reduce_mixed(ins, [a.view for a in accs], accumulate, None, status, out_sizes, dtype=C.DTYPE[ft])
            what2 = f"ft={ft} {name}, {what}, accumulate={accumulate}"
            assert status.tolist() == [1, 0, 1], what2
            assert out_sizes.tolist() == [sizes[0], reported, sizes[2]], what2
            _same(accs[1].bits(), middle, f"{what2}: the failing member's accumulator")
            for k in (0, 2):
                want = R.reduce_expected(fills[k], [src.wide[s][k] for s in range(3)], bool(accumulate))
                _same(accs[k].bits(), C.bits(want), f"{what2}: neighbour {k}")
            assert all(a.guards_intact() for a in accs), what2 + ": guard words overwritten"


# ------------------------------------------------------------------------------------------------------------ routes
def test_routes_agree():
    import dietgpu_amd as dg

    ft, S, raw_at = C.FTS[1], 3, (1,)
    src = R.staging(ft)
    rows, raws = _rows(src, "staging", 10), _raws(src, "staging")
    B = len(src.sizes)
    ins = _ins(rows, raws, S, list(range(B)), raw_at)
    results = []
    try:
        for route in (False, True):
            dg.prefer_torch_ops(route)
            accs = [Acc(n, fill=src.start[i]) for i, n in enumerate(src.sizes)]
            assert dg.decompress_data_reduce_mixed(ins, [a.view for a in accs], True) == 0  # (the float type from the raw row)
            results.append([a.bits() for a in accs])
    finally:
        dg.prefer_torch_ops(True)
    accs = [Acc(n, fill=src.start[i]) for i, n in enumerate(src.sizes)]
    flat = [t for member in ins for t in member]
    kinds = [0 if t.dtype == torch.uint8 else 1 for t in flat]
    assert sum(kinds) == B
    used = ctypes.c_size_t(99)
    rc = dg.lib().dgpu_float_decode_reduce_mixed(
        None, 0, ctypes.byref(used), ft, 10, 1, B, S, (ctypes.c_void_p * (B * S))(*[r.data_ptr() for r in flat]),
        (ctypes.c_uint32 * (B * S))(*[r.numel() * r.element_size() for r in flat]), (ctypes.c_uint8 * (B * S))(*kinds),
        (ctypes.c_void_p * B)(*[a.view.data_ptr() for a in accs]), (ctypes.c_uint32 * B)(*src.sizes), None, None,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and used.value == 0, dg.lib().dgpu_last_error()
    results.append([a.bits() for a in accs])
    want = src.expected(S, True)
    for k in range(B):
        for r, route in zip(results, ("ctypes", "torch op", "C ABI")):
            _same(r[k], C.bits(want[k]), f"{route}: member {k}")


def test_the_torch_op_rejects_a_source_of_another_dtype():
    import dietgpu_amd as dg

    src = R.staging(C.FTS[1])
    rows = _rows(src, "staging", 10)
    a = Acc(src.sizes[0])
    alien = torch.zeros(src.sizes[0], dtype=torch.float16, device=_dev())
    for route in (True, False):
        dg.prefer_torch_ops(route)
        try:
            with pytest.raises(RuntimeError):
                dg.decompress_data_reduce_mixed([[rows[0][0], alien]], [a.view], False, dtype=torch.bfloat16)
        finally:
            dg.prefer_torch_ops(True)
    assert a.guards_intact()


# ------------------------------------------------------------------------------------------------------------- graph
def test_graph_replay_adds_the_sources_in_order():
    import dietgpu_amd as dg

    ft, S, members = C.FTS[1], 3, [0, 1, 5]
    src = R.staging(ft)
    rows, raws = _rows(src, "staging", 10), _raws(src, "staging")
    ins = _ins(rows, raws, S, members, (1,))
    accs = [Acc(src.sizes[i], fill=src.start[i]) for i in members]
    views = [a.view for a in accs]
    status = torch.zeros(len(members), dtype=torch.uint8, device=_dev())

    def call():  # (dtype given: nothing synchronises)
        dg.decompress_data_reduce_mixed(ins, views, True, None, status, None, dtype=C.DTYPE[ft])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # the warm call: makes the parameter block resident
    torch.cuda.synchronize()
    for a, i in zip(accs, members):  # back to the start: the replays alone are measured
        a.view.copy_(torch.from_numpy(src.start[i]))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        call()
    torch.cuda.synchronize()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert status.tolist() == [1] * len(members)
    want = src.expected(S, True, reps=2)  # the start plus the sources, added twice in order (a capture does not execute)
    for a, i in zip(accs, members):
        _same(a.bits(), C.bits(want[i]), f"member {i} after two replays")
        assert a.guards_intact()
    del graph
    dg.lib().dgpu_release_graph_state()
