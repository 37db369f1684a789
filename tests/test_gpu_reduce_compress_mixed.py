"""Reduce-compress with mixed sources on the GPU (dgpu_float_reduce_compress_mixed: k_ans_decode_reduce_mixed_stats,
k_normalize, k_ans_encode_cast): sources that are archives or raw rows of float16 / bfloat16 words are summed into the
float32 accumulators, and the sums are compressed again from the exponent counts the reduce kernel made while it stored
them.  RAW LAST is the case in which those counts are made of sums whose last addend was never decoded.

Inputs and expected accumulators are those of tests/reduce_cases.py, a raw source being the words uploaded instead of
their archive; the expected archives are, byte for byte, dgpu_float_cast_compress of the accumulators the call left."""
import numpy as np
import pytest
import torch

import accum_cases as C
import reduce_cases as R
from test_gpu_accumulate import Acc, _dev
from test_gpu_reduce_compress import FTS, Out, _rows, _same
from test_gpu_reduce_mixed import _ins, _raws

pytestmark = pytest.mark.gpu


def _call(ft, ins, accs, accumulate, prob_bits):
    import dietgpu_amd as dg

    out = Out(ft, [a.n for a in accs])
    comp, csizes, used = dg.decompress_data_reduce_compress_mixed(ins, [a.view for a in accs], accumulate, None, out.status, out.sizes,
                                                                  out.comp, out.csizes, prob_bits=prob_bits, dtype=C.DTYPE[ft])
    assert comp.data_ptr() == out.comp.data_ptr() and csizes.data_ptr() == out.csizes.data_ptr()
    return out, used


def _cast_compress(accs, ft, prob_bits):
    import dietgpu_amd as dg

    comp, sizes, _ = dg.compress_data_cast([a.view for a in accs], C.DTYPE[ft], prob_bits=prob_bits)
    host, n = comp.cpu().numpy(), sizes.tolist()
    return [host[k, : n[k]] for k in range(len(accs))]


def raw_patterns(S):
    """raw last, first and all"""
    seen, out = set(), []
    for name, p in (("last", (S - 1,)), ("first", (0,)), ("all", tuple(range(S)))):
        if p not in seen:
            seen.add(p)
            out.append((name, p))
    return out


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 8])
@pytest.mark.parametrize("prob_bits", C.PROB_BITS)
@pytest.mark.parametrize("ft", FTS)
def test_mixed_reduce_compress_equals_reduce_then_cast_compress(ft, prob_bits, S, accumulate):
    import dietgpu_amd as dg

    src = R.staging(ft)
    rows, raws = _rows(src, "staging", prob_bits), _raws(src, "staging")
    members = list(range(len(src.sizes)))
    B = len(members)
    want = src.expected(S, bool(accumulate))
    for name, raw_at in raw_patterns(S):
        accs = [Acc(src.sizes[i], fill=src.start[i] if accumulate else None) for i in members]
        out, used = _call(ft, _ins(rows, raws, S, members, raw_at), accs, accumulate, prob_bits)
        what = f"ft={ft} probBits={prob_bits} S={S} accumulate={accumulate} raw {name}"
        assert used <= dg.lib().dgpu_float_reduce_compress_temp_bytes(ft, B, max(src.sizes)), what
        assert out.status.tolist() == [1] * B, what
        assert out.sizes.tolist() == list(src.sizes), what
        got_arch = out.archives()
        for k in members:
            _same(accs[k].bits(), C.bits(want[k]), f"{what}: accumulator of member {k}")
            assert accs[k].guards_intact(), f"{what}: member {k}: guard words overwritten"
        for k, cast in enumerate(_cast_compress(accs, ft, prob_bits)):
            _same(got_arch[k], cast, f"{what}: archive of member {k} against dgpu_float_cast_compress of its accumulator")


@pytest.mark.parametrize("ft", FTS)
def test_a_failed_member_writes_a_decodable_archive_and_keeps_its_accumulator(ft):
    """three members of two sources; the middle one fails -- a raw row one word short, a raw row beside an archive that
    is truncated, sources that state fewer words than the capacity: status [1, 0, 1], the middle accumulator (any bits)
    untouched, its archive the flat-table archive of the cast of those bits, the neighbours as in a sound call"""
    import cast_ref
    import dietgpu_amd as dg

    name = "two 4-block tiles"
    _, sizes, _ = C.MALFORMED_BATCHES[name]
    n1 = sizes[1]
    src = R.malformed(ft, name)
    rows, raws = _rows(src, "malformed " + name, 10), _raws(src, "malformed " + name)
    cases = [
        ("raw source 1 one word short", [rows[0][1], raws[1][1][: n1 - 1]], n1, n1),
        ("raw source 0 one word short", [raws[0][1][: n1 - 1], raws[1][1]], n1, n1 - 1),
        ("a truncated archive beside a raw row", [raws[0][1], rows[1][1][: rows[1][1].numel() - 16]], n1, n1),
        ("raw rows of fewer words than the capacity", [raws[0][1], raws[1][1]], n1 + 1, n1),
    ]
    for what, middle_ins, cap1, reported in cases:
        ins = [[raws[0][0], rows[1][0]], middle_ins, [rows[0][2], raws[1][2]]]
        caps = [sizes[0], cap1, sizes[2]]
        for accumulate in (0, 1):
            fills = [R.finite_bits(cap, 20 * k + accumulate) for k, cap in enumerate(caps)]
            middle = R.any_bits(cap1, 7 + accumulate)
            accs = [Acc(cap, fill=f) for cap, f in zip(caps, fills)]
            accs[1].view.view(torch.int32).copy_(torch.from_numpy(middle.view(np.int32)))
            out, _ = _call(ft, ins, accs, accumulate, 10)
            what2 = f"ft={ft} {what}, accumulate={accumulate}"
            assert out.status.tolist() == [1, 0, 1], what2
            assert out.sizes.tolist() == [sizes[0], reported, sizes[2]], what2
            _same(accs[1].bits(), middle, f"{what2}: the failing member's accumulator")
            got_arch = out.archives()
            for k in (0, 2):
                want = R.reduce_expected(fills[k], [src.wide[s][k] for s in range(2)], bool(accumulate))
                _same(accs[k].bits(), C.bits(want), f"{what2}: neighbour {k}")
            cast = _cast_compress(accs, ft, 10)
            for k in (0, 2):
                _same(got_arch[k], cast[k], f"{what2}: archive of neighbour {k}")
            # the failed member's archive decodes to the cast of what the accumulator holds
            dec = torch.empty(cap1, dtype=C.DTYPE[ft], device=_dev())
            st = torch.zeros(1, dtype=torch.uint8, device=_dev())
            dg.decompress_data(True, [out.comp[1, : got_arch[1].size]], [dec], False, None, st, None, prob_bits=10)
            assert st.tolist() == [1], what2
            _same(dec.view(torch.int16).cpu().numpy().view(np.uint16), cast_ref.cast_ref(middle, ft), f"{what2}: the failed member's archive")
            assert all(a.guards_intact() for a in accs), what2
