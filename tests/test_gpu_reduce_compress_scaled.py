"""Scaled reduce-compress on the GPU (dgpu_float_reduce_compress_scaled: k_ans_decode_reduce_mixed_stats_scaled,
k_normalize, k_ans_encode_cast): the float32 sums are multiplied by the call's scale where they are stored, and it is
the SCALED value that is rounded to the archive type, counted for the encoder's table and compressed -- so a mean that
the archive type represents does not overflow because the sum would have.

Expected values are built on the host: tests/reduce_cases.py's expected(S, accumulate) times np.float32(scale), and the
oracle's archive of tests/cast_ref.py's rounding of that product.  Accumulators, archive sizes, archive bytes and the
guard row behind the archives are compared bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import accum_cases as C
import cast_ref
import oracle as O
import reduce_cases as R
from test_gpu_accumulate import Acc, _dev
from test_gpu_reduce_compress import FTS, Out, _rows, _same, _upload, _want_archive
from test_gpu_reduce_mixed import _ins, _raw, _raws
from test_gpu_reduce_scaled import THIRD, scaled

pytestmark = pytest.mark.gpu


def _call(ft, ins, accs, accumulate, prob_bits, scale):
    import dietgpu_amd as dg

    mixed = any(t.dtype != torch.uint8 for member in ins for t in member)
    f = dg.decompress_data_reduce_compress_mixed if mixed else dg.decompress_data_reduce_compress
    out = Out(ft, [a.n for a in accs])
    comp, csizes, used = f(ins, [a.view for a in accs], accumulate, None, out.status, out.sizes, out.comp, out.csizes, prob_bits=prob_bits,
                           dtype=C.DTYPE[ft], scale=scale)
    assert comp.data_ptr() == out.comp.data_ptr() and csizes.data_ptr() == out.csizes.data_ptr()
    return out, used


_SOURCES = {"staging": R.staging, "orders67x4": lambda ft: R.orders(ft, 67, 4)}


@functools.lru_cache(maxsize=None)
def _want(tag, ft, S, accumulate, prob_bits, scale):
    """per member of the case `tag`: (the scaled sum's bits, the archive of its rounding), computed once"""
    src = _SOURCES[tag](ft)
    bits = [C.bits(scaled(w, scale)) for w in src.expected(S, bool(accumulate))]
    return bits, [_want_archive(ft, b, prob_bits) for b in bits]


def _run_and_check(tag, ft, S, prob_bits, accumulate, raw_at, scale, what, pair=False):
    import dietgpu_amd as dg

    src = _SOURCES[tag](ft)
    rows, raws = _rows(src, tag, prob_bits), _raws(src, tag)
    members = list(range(len(src.sizes)))
    B = len(members)
    ins = _ins(rows, raws, S, members, raw_at)
    accs = [Acc(src.sizes[i], fill=src.start[i] if accumulate else None) for i in members]
    out, used = _call(ft, ins, accs, accumulate, prob_bits, scale)
    what = f"ft={ft} probBits={prob_bits} S={S} accumulate={accumulate} raw at {list(raw_at)} scale={scale} {what}"
    need = dg.lib().dgpu_float_reduce_compress_temp_bytes(ft, B, max(src.sizes))
    assert used <= need, what
    assert out.status.tolist() == [1] * B, what
    assert out.sizes.tolist() == list(src.sizes), what
    want_bits, want_arch = _want(tag, ft, S, accumulate, prob_bits, scale)
    got_arch = out.archives()  # (checks the guard row behind the archives)
    for k in members:
        _same(accs[k].bits(), want_bits[k], f"{what}: accumulator of member {k} ({src.sizes[k]} words)")
        assert accs[k].guards_intact(), f"{what}: member {k}: guard words overwritten"
        assert got_arch[k].size == want_arch[k].size, f"{what}: archive size of member {k}"
        _same(got_arch[k], want_arch[k], f"{what}: archive of member {k}")
    if pair:
        seq = [Acc(src.sizes[i], fill=src.start[i] if accumulate else None) for i in members]
        st = torch.zeros(B, dtype=torch.uint8, device=_dev())
        dg.decompress_data_reduce(_ins(rows, raws, S, members, ()), [a.view for a in seq], accumulate, None, st, None, prob_bits=prob_bits,
                                  dtype=C.DTYPE[ft], scale=scale)
        assert st.tolist() == [1] * B, what
        comp2, sizes2, _ = dg.compress_data_cast([a.view for a in seq], C.DTYPE[ft], prob_bits=prob_bits)
        host2, n2 = comp2.cpu().numpy(), sizes2.tolist()
        for k in members:
            _same(accs[k].bits(), seq[k].bits(), f"{what}: accumulator of member {k} against decompress_data_reduce(scale)")
            _same(got_arch[k], host2[k, : n2[k]], f"{what}: archive of member {k} against compress_data_cast")
    return used, need


def raw_patterns(S):
    """raw sources: none, the last, all"""
    seen, out = set(), []
    for name, p in (("none", ()), ("last", (S - 1,)), ("all", tuple(range(S)))):
        if p not in seen:
            seen.add(p)
            out.append((name, p))
    return out


# ------------------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 8])
@pytest.mark.parametrize("ft", FTS)
def test_the_archive_is_that_of_the_scaled_sum(ft, S, accumulate):
    for scale in (THIRD, 0.5):
        for name, raw_at in raw_patterns(S):
            _run_and_check("staging", ft, S, 10, accumulate, raw_at, scale, f"staging shapes, raw {name}",
                           pair=(S == 2 and accumulate == 1 and scale == THIRD and name == "none"))


def test_table_precision_eleven():
    _run_and_check("staging", O.FLOAT16, 2, 11, 1, (), THIRD, "staging shapes")
    _run_and_check("staging", O.FLOAT16, 2, 11, 0, (1,), THIRD, "staging shapes")


@pytest.mark.parametrize("ft", FTS)
def test_counts_in_temp_memory(ft):
    """67 members: more than the stream's counters hold, so the counts of the scaled sums live in temp memory"""
    for accumulate, raw_at in ((0, ()), (1, (1,))):
        used, need = _run_and_check("orders67x4", ft, 2, 10, accumulate, raw_at, THIRD, "67 members of 4-block tiles")
        assert 0 < used <= need


# --------------------------------------------------------------------------------------- what the feature exists for
def test_a_mean_that_is_representable_does_not_overflow():
    """two float16 sources of 40000.0: their sum, 80000, is +inf as float16; their mean is 40000.  With scale 0.5 the
    accumulator holds 40000.0f and the archive decodes to float16 40000 in every word; with scale 1 it decodes to +inf."""
    import dietgpu_amd as dg

    ft, n = O.FLOAT16, R.ORDER_WORDS
    words = R.constant_words(ft, 40000.0)
    archive, raw = _upload(O.float_compress(ft, words, 10)), _raw(ft, words)
    for ins in ([archive, archive], [archive, raw]):
        for scale, acc_want, word_want in ((0.5, 40000.0, int(words[0])), (1.0, 80000.0, 0x7C00)):
            a = Acc(n)
            out, _ = _call(ft, [ins], [a], 0, 10, scale)
            assert out.status.tolist() == [1] and out.sizes.tolist() == [n]
            assert (a.bits().view(np.float32) == np.float32(acc_want)).all() and a.guards_intact()
            got = out.archives()[0]
            _same(got, O.float_compress(ft, np.full(n, word_want, np.uint16), 10), f"scale {scale}: the archive")
            dec = torch.empty(n, dtype=torch.float16, device=_dev())
            st = torch.zeros(1, dtype=torch.uint8, device=_dev())
            dg.decompress_data(True, [out.comp[0, : got.size]], [dec], False, None, st, None)
            assert st.tolist() == [1]
            assert (dec.view(torch.int16).cpu().numpy().view(np.uint16) == word_want).all(), f"scale {scale}"
            assert bool(torch.isinf(dec).all()) == (scale == 1.0)


# --------------------------------------------------------------------------------------------------- all or nothing
@pytest.mark.parametrize("ft", FTS)
def test_a_failed_member_keeps_its_accumulator_and_its_archive_decodes(ft):
    """three members of two sources; the middle one fails: status [1, 0, 1], its accumulator (any bits) untouched and NOT
    scaled, its archive decodable to the cast of those bits; the neighbours scaled, and their archives those of the
    scaled sums"""
    import dietgpu_amd as dg

    name = "two 4-block tiles"
    _, sizes, _ = C.MALFORMED_BATCHES[name]
    n1 = sizes[1]
    src = R.malformed(ft, name)
    rows, raws = _rows(src, "malformed " + name, 10), _raws(src, "malformed " + name)
    cases = [
        ("a truncated archive", [rows[0][1], rows[1][1][: rows[1][1].numel() - 16]], n1, n1),
        ("raw source 1 one word short", [rows[0][1], raws[1][1][: n1 - 1]], n1, n1),
        ("sources of fewer words than the capacity", [rows[0][1], rows[1][1]], n1 + 1, n1),
    ]
    for what, middle_ins, cap1, reported in cases:
        ins = [[rows[0][0], rows[1][0]], middle_ins, [rows[0][2], raws[1][2]]]
        caps = [sizes[0], cap1, sizes[2]]
        for accumulate in (0, 1):
            fills = [R.finite_bits(cap, 20 * k + accumulate) for k, cap in enumerate(caps)]
            middle = R.any_bits(cap1, 7 + accumulate)
            accs = [Acc(cap, fill=f) for cap, f in zip(caps, fills)]
            accs[1].view.view(torch.int32).copy_(torch.from_numpy(middle.view(np.int32)))
            out, _ = _call(ft, ins, accs, accumulate, 10, THIRD)
            what2 = f"ft={ft} {what}, accumulate={accumulate}"
            assert out.status.tolist() == [1, 0, 1], what2
            assert out.sizes.tolist() == [sizes[0], reported, sizes[2]], what2
            _same(accs[1].bits(), middle, f"{what2}: the failing member's accumulator")
            got_arch = out.archives()
            for k in (0, 2):
                want = C.bits(scaled(R.reduce_expected(fills[k], [src.wide[s][k] for s in range(2)], bool(accumulate)), THIRD))
                _same(accs[k].bits(), want, f"{what2}: neighbour {k}")
                _same(got_arch[k], _want_archive(ft, want, 10), f"{what2}: archive of neighbour {k}")
            dec = torch.empty(cap1, dtype=C.DTYPE[ft], device=_dev())
            st = torch.zeros(1, dtype=torch.uint8, device=_dev())
            dg.decompress_data(True, [out.comp[1, : got_arch[1].size]], [dec], False, None, st, None, prob_bits=10)
            assert st.tolist() == [1], what2
            _same(dec.view(torch.int16).cpu().numpy().view(np.uint16), cast_ref.cast_ref(middle, ft), f"{what2}: the failed member's archive")
            assert all(a.guards_intact() for a in accs), what2


# ------------------------------------------------------------------------------------------------------------ routes
def test_routes_agree():
    """the ctypes route, the torch op, and the C ABI with sourceKind NULL and optional outputs NULL"""
    import dietgpu_amd as dg

    ft, S = O.BFLOAT16, 2
    src = R.staging(ft)
    rows, raws = _rows(src, "staging", 10), _raws(src, "staging")
    B = len(src.sizes)
    members = list(range(B))
    want_bits, want_arch = _want("staging", ft, S, 1, 10, THIRD)
    if dg.ops._fast_ops(10) is not None:
        assert hasattr(torch.ops.dietgpu_amd, "decompress_data_reduce_compress_scaled")
    try:
        for route in (False, True):
            dg.prefer_torch_ops(route)
            accs = [Acc(n, fill=src.start[i]) for i, n in enumerate(src.sizes)]
            out, _ = _call(ft, _ins(rows, raws, S, members, (1,)), accs, 1, 10, THIRD)
            got_arch = out.archives()
            for k in members:
                _same(accs[k].bits(), want_bits[k], f"torch ops {route}: accumulator {k}")
                _same(got_arch[k], want_arch[k], f"torch ops {route}: archive {k}")
    finally:
        dg.prefer_torch_ops(True)
    flat = [rows[s][i] for i in members for s in range(S)]
    accs = [Acc(n, fill=src.start[i]) for i, n in enumerate(src.sizes)]
    out = Out(ft, src.sizes)
    need = dg.lib().dgpu_float_reduce_compress_temp_bytes(ft, B, max(src.sizes))
    temp = torch.empty(need, dtype=torch.uint8, device=_dev())
    used = ctypes.c_size_t(0)
    rc = dg.lib().dgpu_float_reduce_compress_scaled(
        ctypes.c_void_p(temp.data_ptr()), need, ctypes.byref(used), ft, 10, 1, B, S, (ctypes.c_void_p * (B * S))(*[r.data_ptr() for r in flat]),
        (ctypes.c_uint32 * (B * S))(*[r.numel() for r in flat]), None, THIRD, (ctypes.c_void_p * B)(*[a.view.data_ptr() for a in accs]),
        (ctypes.c_uint32 * B)(*src.sizes), (ctypes.c_void_p * B)(*[out.comp[k].data_ptr() for k in range(B)]), None, None, None,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and used.value <= need, dg.lib().dgpu_last_error()
    host = out.comp.cpu().numpy()
    for k in members:
        _same(accs[k].bits(), want_bits[k], f"C ABI: accumulator {k}")
        _same(host[k, : want_arch[k].size], want_arch[k], f"C ABI: archive {k}")
