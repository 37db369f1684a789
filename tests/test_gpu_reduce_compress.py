"""Reduce-compress on the GPU (dgpu_float_reduce_compress: k_ans_decode_reduce_stats, k_normalize, k_ans_encode_cast):
S float16 / bfloat16 archives per float32 accumulator summed left to right, and the sum -- rounded to the archive type --
compressed again by the same call, from the exponent counts the reduce kernel made while it stored the sums.

The inputs are the cases of tests/reduce_cases.py; the source archives are the CPU oracle's.  Every expected value is
built on the host: accumulators by numpy float32 adds in source order, archives as the oracle's compression of
tests/cast_ref.py's rounding of those accumulators.  Everything is compared BIT FOR BIT -- every accumulator word, every
archive byte up to the reported size, the guard words around the accumulators and the guard row behind the archives --
and, where the test says so, with decompress_data_reduce followed by compress_data_cast run on copies."""
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

pytestmark = pytest.mark.gpu

FTS = (O.FLOAT16, O.BFLOAT16)  # the archive types of a cast
ROW_GUARD = 0xA5

_gpu_cache = {}


def _gpu(key, make):
    if key not in _gpu_cache:
        _gpu_cache[key] = make()
    return _gpu_cache[key]


def _upload(archive):
    return torch.from_numpy(archive.copy()).to(_dev())


def _rows(src, tag, prob_bits):
    """[source][element] archives of `src` on the GPU, uploaded once"""
    return _gpu((tag, src.ft, prob_bits), lambda: [[_upload(a) for a in row] for row in src.archives(prob_bits)])


def _same(got, want, what):
    assert got.size == want.size, f"{what}: {got.size} against {want.size}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, the first at {bad[:4].tolist()}"


def _want_archive(ft, acc_bits, prob_bits):
    """what cast-compress writes for an accumulator of these bits: the oracle's archive of the rounded words"""
    return O.float_compress(ft, cast_ref.cast_ref(acc_bits, ft), prob_bits)


@functools.lru_cache(maxsize=None)
def _want_archives(tag, ft, S, accumulate, prob_bits):
    """the expected archives of every member of the case `tag`, computed once"""
    src = _SOURCES[tag](ft)
    return [_want_archive(ft, C.bits(w), prob_bits) for w in src.expected(S, bool(accumulate))]


_SOURCES = {"staging": R.staging}
for _lead in (0, 3):
    _SOURCES[f"tails{_lead}"] = lambda ft, lead=_lead: R.tails(ft, lead)
for _B in (13, 67):
    for _tb in C.ORDER_GEOMETRIES:
        _SOURCES[f"orders{_B}x{_tb}"] = lambda ft, B=_B, tb=_tb: R.orders(ft, B, tb)


class Out:
    """the outputs of one call: status and sizes with poison values, the archive matrix with a guard row behind it"""

    def __init__(self, ft, caps):
        n = len(caps)
        self.n = n
        self.cols = max(O.float_max_compressed_size(ft, max(caps)), 16)
        self.status = torch.full((n,), 7, dtype=torch.uint8, device=_dev())
        self.sizes = torch.full((n,), -7, dtype=torch.int32, device=_dev())
        self.comp = torch.full((n + 1, self.cols), ROW_GUARD, dtype=torch.uint8, device=_dev())
        self.csizes = torch.full((n + 1,), -7, dtype=torch.int32, device=_dev())

    def archives(self):
        host, sizes = self.comp.cpu().numpy(), self.csizes.tolist()
        assert (host[self.n] == ROW_GUARD).all() and sizes[self.n] == -7, "the row behind the archives was written"
        assert all(0 < s <= self.cols for s in sizes[: self.n]), sizes
        return [host[i, : sizes[i]] for i in range(self.n)]


def _call(ft, ins, accs, accumulate, prob_bits, temp=None):
    import dietgpu_amd as dg

    out = Out(ft, [a.n for a in accs])
    comp, csizes, used = dg.decompress_data_reduce_compress(ins, [a.view for a in accs], accumulate, temp, out.status, out.sizes, out.comp,
                                                            out.csizes, prob_bits=prob_bits, dtype=C.DTYPE[ft])
    assert comp.data_ptr() == out.comp.data_ptr() and csizes.data_ptr() == out.csizes.data_ptr()
    return out, used


def _accs(src, members, accumulate, offsets=None):
    return [Acc(src.sizes[i], offsets[k] if offsets else 0, fill=src.start[i] if accumulate else None) for k, i in enumerate(members)]


def _run_and_check(tag, ft, S, prob_bits, members, accumulate, what, offsets=None, pair=False, decode=False):
    """one call for `members` of the case `tag` with the first S sources: status, word sizes, every accumulator word, the
    guards, archive sizes and bytes; `pair`: decompress_data_reduce + compress_data_cast on copies leave the same;
    `decode`: the archives decode to the rounded sums"""
    import dietgpu_amd as dg

    src = _SOURCES[tag](ft)
    rows = _rows(src, tag, prob_bits)
    B = len(members)
    ins = [[rows[s][i] for s in range(S)] for i in members]
    accs = _accs(src, members, accumulate, offsets)
    out, used = _call(ft, ins, accs, accumulate, prob_bits)
    what = f"ft={ft} probBits={prob_bits} S={S} accumulate={accumulate} {what}"
    assert used <= dg.lib().dgpu_float_reduce_compress_temp_bytes(ft, B, max(src.sizes[i] for i in members)), what
    assert out.status.tolist() == [1] * B, what
    assert out.sizes.tolist() == [src.sizes[i] for i in members], what
    want = src.expected(S, bool(accumulate))
    want_arch = _want_archives(tag, ft, S, accumulate, prob_bits)
    got = [a.bits() for a in accs]
    got_arch = out.archives()
    for k, i in enumerate(members):
        _same(got[k], C.bits(want[i]), f"{what}: accumulator of member {k} ({src.sizes[i]} words)")
        assert accs[k].guards_intact(), f"{what}: member {k}: guard words overwritten"
        _same(got_arch[k], want_arch[i], f"{what}: archive of member {k} ({src.sizes[i]} words)")
    if pair:
        seq = _accs(src, members, accumulate, offsets)
        st = torch.zeros(B, dtype=torch.uint8, device=_dev())
        dg.decompress_data_reduce(ins, [a.view for a in seq], accumulate, None, st, None, prob_bits=prob_bits, dtype=C.DTYPE[ft])
        assert st.tolist() == [1] * B, what
        comp2, sizes2, _ = dg.compress_data_cast([a.view for a in seq], C.DTYPE[ft], prob_bits=prob_bits)
        host2, n2 = comp2.cpu().numpy(), sizes2.tolist()
        for k in range(B):
            _same(got[k], seq[k].bits(), f"{what}: accumulator of member {k} against decompress_data_reduce")
            _same(got_arch[k], host2[k, : n2[k]], f"{what}: archive of member {k} against compress_data_cast")
    if decode:
        outs = [torch.empty(src.sizes[i], dtype=C.DTYPE[ft], device=_dev()) for i in members]
        st = torch.zeros(B, dtype=torch.uint8, device=_dev())
        dg.decompress_data(True, [out.comp[k, : a.size] for k, a in enumerate(got_arch)], outs, False, None, st, None, prob_bits=prob_bits)
        assert st.tolist() == [1] * B, what
        for k, i in enumerate(members):
            _same(outs[k].view(torch.int16).cpu().numpy().view(np.uint16), cast_ref.cast_ref(C.bits(want[i]), ft),
                  f"{what}: decoded archive of member {k}")


# ------------------------------------------------------------------------------------------------------ 1. equivalence
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("prob_bits", C.PROB_BITS)
@pytest.mark.parametrize("ft", FTS)
def test_one_call_equals_reduce_then_cast_compress(ft, prob_bits, S, accumulate):
    """the staging shapes (16- and 4-block tiles, whole, ring, mixed and boundary waves, an odd block count, partial last
    blocks): the host's sums and the oracle's archives of their rounding, and the two calls this one replaces"""
    src = R.staging(ft)
    _run_and_check("staging", ft, S, prob_bits, list(range(len(src.sizes))), accumulate, "staging shapes", pair=True,
                   decode=(prob_bits == 10 and S == 3 and accumulate == 1))


# ----------------------------------------------------------------------------------------------- 2. tails and alignment
@pytest.mark.parametrize("lead", [0, 3])
@pytest.mark.parametrize("ft", FTS)
def test_partial_last_blocks_count_the_words_below_n(ft, lead):
    """the row-wise store path; accumulators at word offsets 0..3"""
    src = R.tails(ft, lead)
    members = list(range(len(src.sizes)))
    for accumulate in (0, 1):
        _run_and_check(f"tails{lead}", ft, 2, 10, members, accumulate, f"lead {lead}", offsets=[i % 4 for i in members])


# --------------------------------------------------------------------------------------------------------- 3. geometry
@pytest.mark.parametrize("B", [13, 67])
@pytest.mark.parametrize("ft", FTS)
def test_workgroup_orders_work_lists_and_both_count_paths(ft, B):
    """B = 13: the counts in the stream's counters; B = 67: in temp memory, cleared on the stream"""
    import dietgpu_amd as dg

    L = dg.lib()
    for tile_blocks in C.ORDER_GEOMETRIES:
        tag = f"orders{B}x{tile_blocks}"
        src = R.orders(ft, B, tile_blocks)
        members = list(range(B))
        assert -(-max(src.sizes) // C.BLK) == C.ORDER_GEOMETRIES[tile_blocks][1]  # this geometry, two tiles per member
        for order in (0, 1, 2):
            L.dgpu_debug_set_decoder_order(order)
            try:
                for accumulate in (0, 1):
                    _run_and_check(tag, ft, 2, 10, members, accumulate, f"order {order}, {tile_blocks}-block tiles")
            finally:
                L.dgpu_debug_set_decoder_order(-1)
        for lists in (1, 0):
            L.dgpu_debug_set_work_lists(lists)
            try:
                for accumulate in (0, 1):
                    _run_and_check(tag, ft, 2, 10, members, accumulate, f"work lists {lists}, {tile_blocks}-block tiles")
            finally:
                L.dgpu_debug_set_work_lists(-1)


# --------------------------------------------------------------------------------------------- 4. rounding at the edges
@pytest.mark.parametrize("ft", FTS)
def test_rounding_edges_are_counted_as_the_encoder_rounds_them(ft):
    """the accumulator starts as every edge of the two conversions (ties both ways, carries into the exponent, overflow,
    denormals, NaNs), one source of +0.0 words is added: the archive is the oracle's of the reference rounding of the
    numpy sum.  NaN words are compared in the archive only, where the cast makes them canonical; what payload an add
    leaves in the accumulator is the hardware's business."""
    n = 2 * C.BLK + 77
    start = np.resize(cast_ref.EDGE_BITS, n).astype(np.uint32)
    zeros = _gpu(("zeros", ft), lambda: _upload(O.float_compress(ft, np.zeros(n, np.uint16), 10)))
    a = Acc(n)
    a.view.view(torch.int32).copy_(torch.from_numpy(start.view(np.int32)))
    out, _ = _call(ft, [[zeros]], [a], 1, 10)
    assert out.status.tolist() == [1] and out.sizes.tolist() == [n]
    with np.errstate(invalid="ignore"):
        want = (start.view(np.float32) + np.zeros(n, np.float32)).astype(np.float32).view(np.uint32)
    got = a.bits()
    nan = np.isnan(want.view(np.float32))
    assert nan.any() and (want[~nan] != start[~nan]).any()  # (-0.0 + +0.0 is +0.0)
    _same(got[~nan], want[~nan], f"ft={ft}: accumulator, the words that are not NaN")
    assert np.isnan(got.view(np.float32)[nan]).all() and ((got[nan] ^ want[nan]) >> 31 == 0).all()
    assert a.guards_intact()
    _same(out.archives()[0], _want_archive(ft, want, 10), f"ft={ft}: archive")


# ------------------------------------------------------------------------------------------------- 5. all or nothing
def _failure_cases(ft, name, src):
    """-> [(what, {source: (archive, bytes offered or None)}, capacity of the middle member, size reported)]"""
    tile_blocks, sizes, _ = C.MALFORMED_BATCHES[name]
    n1 = sizes[1]
    out = []
    for s in range(3):
        good = src.archives(10)[s][1]
        for what, bad in C.corruptions(ft, good, n1, tile_blocks):
            out.append((f"source {s}: {what}", {s: (bad, None)}, n1, n1))
        out.append((f"source {s}: truncated by 16 bytes through inBytes", {s: (good, good.size - 16)}, n1, n1))
        other = O.float_compress(ft, src.words[s][1][: n1 - 5], 10)
        out.append((f"source {s}: another word count", {s: (other, None)}, n1, n1 - 5 if s == 0 else n1))
        other_ft = FTS[1 - FTS.index(ft)]
        alien = O.float_compress(other_ft, C.words(other_ft, "c" * (n1 // C.BLK), n1 % C.BLK, "c", seed=4242 + s), 10)
        out.append((f"source {s}: float type {other_ft}", {s: (alien, None)}, n1, n1))
    out.append(("capacity one word short", {}, n1 - 1, n1))
    # well-formed sources that agree with each other but state fewer words than the capacity: the new rule of this call
    short = {s: (O.float_compress(ft, src.words[s][1][: n1 - 5], 10), None) for s in range(3)}
    out.append(("every source five words short of the capacity", short, n1, n1 - 5))
    return out


@pytest.mark.parametrize("name", list(C.MALFORMED_BATCHES))
@pytest.mark.parametrize("ft", FTS)
def test_a_failing_member_keeps_its_bits_and_gets_a_decodable_archive(ft, name):
    """three members, three sources each; the middle member fails (one bad source, a short capacity, short sources):
    status [1, 0, 1], its accumulator as it was, its archive inside the bound and decodable to the rounding of what the
    accumulator holds; the neighbours summed and compressed as if it were not there"""
    import dietgpu_amd as dg

    _, sizes, _ = C.MALFORMED_BATCHES[name]
    src = R.malformed(ft, name)
    rows = _rows(src, "malformed " + name, 10)
    fills = {acc: [R.finite_bits(cap, 10 * k + acc) for k, cap in enumerate(sizes)] for acc in (0, 1)}
    neighbours = {}  # (accumulate, k) -> (sum, archive), computed once
    for accumulate in (0, 1):
        for k in (0, 2):
            w = R.reduce_expected(fills[accumulate][k], [src.wide[s][k] for s in range(3)], bool(accumulate))
            neighbours[accumulate, k] = (C.bits(w), _want_archive(ft, C.bits(w), 10))
    for what, bad, cap1, reported in _failure_cases(ft, name, src):
        ins = [[rows[s][i] for s in range(3)] for i in range(3)]
        for s, (archive, offered) in bad.items():
            t = _upload(archive)
            ins[1][s] = t[:offered] if offered is not None else t
        caps = [sizes[0], cap1, sizes[2]]
        for accumulate in (0, 1):
            middle = R.any_bits(cap1, 3 + accumulate)
            assert np.isnan(middle.view(np.float32)).any()
            accs = [Acc(caps[0], fill=fills[accumulate][0]), Acc(cap1), Acc(caps[2], fill=fills[accumulate][2])]
            accs[1].view.view(torch.int32).copy_(torch.from_numpy(middle.view(np.int32)))
            out, _ = _call(ft, ins, accs, accumulate, 10)
            what2 = f"ft={ft} {name}, {what}, accumulate={accumulate}"
            assert out.status.tolist() == [1, 0, 1], what2
            assert out.sizes.tolist() == [sizes[0], reported, sizes[2]], what2
            _same(accs[1].bits(), middle, f"{what2}: the failing member's accumulator")
            got_arch = out.archives()
            for k in (0, 2):
                _same(accs[k].bits(), neighbours[accumulate, k][0], f"{what2}: accumulator of neighbour {k}")
                _same(got_arch[k], neighbours[accumulate, k][1], f"{what2}: archive of neighbour {k}")
            assert all(a.guards_intact() for a in accs), what2 + ": guard words overwritten"
            assert got_arch[1].size <= dg.max_float_compressed_size(torch.empty(0, dtype=C.DTYPE[ft]), cap1), what2
            dec = torch.empty(cap1, dtype=C.DTYPE[ft], device=_dev())
            st = torch.zeros(1, dtype=torch.uint8, device=_dev())
            dg.decompress_data(True, [out.comp[1, : got_arch[1].size]], [dec], False, None, st, None)
            assert st.tolist() == [1], what2 + ": the failing member's archive does not decode"
            _same(dec.view(torch.int16).cpu().numpy().view(np.uint16), cast_ref.cast_ref(middle, ft),
                  f"{what2}: the failing member's archive, decoded")


# ------------------------------------------------------------------------------------------------------------ 6. empty
@pytest.mark.parametrize("ft", FTS)
def test_a_member_without_words_among_others(ft):
    import dietgpu_amd as dg

    src = R.staging(ft)
    rows = _rows(src, "staging", 10)
    empty = _gpu(("empty", ft), lambda: _upload(O.float_compress(ft, np.zeros(0, np.uint16), 10)))
    members = [1, None, 2]
    for accumulate in (0, 1):
        ins = [[empty, empty] if i is None else [rows[s][i] for s in range(2)] for i in members]
        accs = [Acc(0) if i is None else Acc(src.sizes[i], fill=src.start[i] if accumulate else None) for i in members]
        out, _ = _call(ft, ins, accs, accumulate, 10)
        assert out.status.tolist() == [1, 1, 1]
        assert out.sizes.tolist() == [src.sizes[1], 0, src.sizes[2]]
        got_arch = out.archives()
        want, want_arch = src.expected(2, bool(accumulate)), _want_archives("staging", ft, 2, accumulate, 10)
        for k, i in enumerate(members):
            assert accs[k].guards_intact()
            if i is not None:
                _same(accs[k].bits(), C.bits(want[i]), f"ft={ft} accumulate={accumulate}: accumulator of member {k}")
                _same(got_arch[k], want_arch[i], f"ft={ft} accumulate={accumulate}: archive of member {k}")
        _same(got_arch[1], O.float_compress(ft, np.zeros(0, np.uint16), 10), f"ft={ft}: the empty member's archive")
        comp2, sizes2, _ = dg.compress_data_cast([a.view for a in accs], C.DTYPE[ft])
        _same(got_arch[1], comp2[1, : int(sizes2[1])].cpu().numpy(), f"ft={ft}: the empty member against compress_data_cast")


# ------------------------------------------------------------------------------------- 7. repeat, counters at rest
def test_three_calls_then_a_histogram_that_shares_the_counters():
    """the counts of the members live in the stream's zero-at-rest counters, which the accumulate-by-atomics histogram of
    a single large tensor uses too: after three calls they are zero again, or that tensor's table would be wrong"""
    import dietgpu_amd as dg

    ft = O.BFLOAT16
    src = R.staging(ft)
    members = list(range(len(src.sizes)))
    for rep in range(3):
        _run_and_check("staging", ft, 3, 10, members, 1, f"call {rep}")
    n = 9 * 1024 * 1024 + 123  # 18 MiB: more than 256 histogram workgroups of 64 KiB, so the counters are used
    words = (np.random.default_rng(5).standard_normal(n).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    t = torch.from_numpy(words.view(np.int16)).to(_dev()).view(torch.bfloat16)
    comp, sizes, _ = dg.compress_data(True, [t])
    _same(comp[0, : int(sizes[0])].cpu().numpy(), O.float_compress(ft, words, 10), "the large tensor after three reduce-compress calls")
    _run_and_check("staging", ft, 3, 10, members, 1, "after the large tensor")


# ------------------------------------------------------------------------------------------- 8. temp memory and routes
@pytest.mark.parametrize("B", [13, 67])
def test_temp_memory_none_and_exactly_the_query(B):
    import dietgpu_amd as dg

    ft, tag = O.BFLOAT16, f"orders{B}x4"
    src = R.orders(ft, B, 4)
    rows = _rows(src, tag, 10)
    members = list(range(B))
    ins = [[rows[s][i] for s in range(2)] for i in members]
    need = dg.lib().dgpu_float_reduce_compress_temp_bytes(ft, B, max(src.sizes))
    want, want_arch = src.expected(2, True), _want_archives(tag, ft, 2, 1, 10)
    results = []
    try:
        for route in (True, False):
            dg.prefer_torch_ops(route)
            for temp in (None, torch.empty(need, dtype=torch.uint8, device=_dev())):
                accs = _accs(src, members, 1)
                out, used = _call(ft, ins, accs, 1, 10, temp)
                assert 0 < used <= need, (route, temp is None, used, need)
                assert out.status.tolist() == [1] * B
                results.append((route, temp is None, [a.bits() for a in accs], out.archives()))
    finally:
        dg.prefer_torch_ops(True)
    for route, no_temp, bits, arch in results:
        for k in members:
            _same(bits[k], C.bits(want[k]), f"torch ops {route}, temp None {no_temp}: accumulator {k}")
            _same(arch[k], want_arch[k], f"torch ops {route}, temp None {no_temp}: archive {k}")


def test_the_c_abi_with_null_optional_outputs():
    import dietgpu_amd as dg

    ft, S = O.FLOAT16, 3
    src = R.staging(ft)
    rows = _rows(src, "staging", 10)
    B = len(src.sizes)
    flat = [rows[s][i] for i in range(B) for s in range(S)]
    accs = _accs(src, list(range(B)), 1)
    out = Out(ft, src.sizes)
    used = ctypes.c_size_t(99)
    rc = dg.lib().dgpu_float_reduce_compress(
        None, 0, ctypes.byref(used), ft, 10, 1, B, S, (ctypes.c_void_p * (B * S))(*[r.data_ptr() for r in flat]),
        (ctypes.c_uint32 * (B * S))(*[r.numel() for r in flat]), (ctypes.c_void_p * B)(*[a.view.data_ptr() for a in accs]),
        (ctypes.c_uint32 * B)(*src.sizes), (ctypes.c_void_p * B)(*[out.comp[k].data_ptr() for k in range(B)]), None, None, None,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, dg.lib().dgpu_last_error()
    want, want_arch = src.expected(S, True), _want_archives("staging", ft, S, 1, 10)
    host = out.comp.cpu().numpy()
    for k in range(B):
        _same(accs[k].bits(), C.bits(want[k]), f"accumulator {k}")
        _same(host[k, : want_arch[k].size], want_arch[k], f"archive {k}")


# ------------------------------------------------------------------------------------------------------------ 9. graph
def test_graph_replay_sums_and_compresses_again():
    import dietgpu_amd as dg

    ft, S, members = O.BFLOAT16, 3, [0, 1, 5]
    src = R.staging(ft)
    rows = _rows(src, "staging", 10)
    ins = [[rows[s][i] for s in range(S)] for i in members]
    accs = [Acc(src.sizes[i], fill=src.start[i]) for i in members]
    views = [a.view for a in accs]
    out = Out(ft, [src.sizes[i] for i in members])
    temp = torch.empty(dg.lib().dgpu_float_reduce_compress_temp_bytes(ft, len(members), max(a.n for a in accs)), dtype=torch.uint8, device=_dev())

    def call():  # (dtype given: reading the header would synchronise, which a capture cannot hold)
        dg.decompress_data_reduce_compress(ins, views, True, temp, out.status, out.sizes, out.comp, out.csizes, dtype=C.DTYPE[ft])

    def refill():
        for a, i in zip(accs, members):
            a.view.copy_(torch.from_numpy(src.start[i]))
        out.comp[: out.n].fill_(0)
        out.csizes.fill_(-7)
        out.status.fill_(7)
        torch.cuda.synchronize()

    want, want_arch = src.expected(S, True), _want_archives("staging", ft, S, 1, 10)
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call()  # the warm call: parameter blocks resident, the stream's counters exist
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            call()
        torch.cuda.synchronize()
        for replay in range(2):
            refill()
            graph.replay()
            torch.cuda.synchronize()
            assert out.status.tolist() == [1] * len(members)
            got_arch = out.archives()
            for k, i in enumerate(members):
                _same(accs[k].bits(), C.bits(want[i]), f"replay {replay}: accumulator of member {i}")
                _same(got_arch[k], want_arch[i], f"replay {replay}: archive of member {i}")
                assert accs[k].guards_intact()
        del graph
    finally:
        dg.lib().dgpu_release_graph_state()
