"""Decode-reduce on the GPU (dgpu_float_decode_reduce, k_ans_decode_reduce): S float archives per float32 accumulator,
summed left to right in one launch, all or nothing per accumulator.

The inputs are the cases of tests/accum_cases.py with further sources beside them (tests/reduce_cases.py); the archives
are the CPU oracle's.  Every expected value is built on the host -- the exact widening and one numpy float32 add per
source, in source order -- and compared BIT FOR BIT on uint32 views, every word of it."""
import ctypes
import os

import numpy as np
import pytest
import torch

import accum_cases as C
import oracle as O
import reduce_cases as R
from test_gpu_accumulate import SENTINEL, Acc, _dev, _free_port

pytestmark = pytest.mark.gpu

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
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} words differ, the first at {bad[:4].tolist()}"


def _reduce_and_check(src, rows, S, prob_bits, members, accumulate, what, offsets=None, sequence=False):
    """one reduce call for `members` with the first S sources: status, sizes, every accumulator word, the guards; with
    `sequence`, S successive decode-accumulate calls on a copy of the accumulators must leave the same bits"""
    import dietgpu_amd as dg

    B = len(members)
    accs = [Acc(src.sizes[i], offsets[k] if offsets else 0, fill=src.start[i] if accumulate else None) for k, i in enumerate(members)]
    status = torch.full((B,), 7, dtype=torch.uint8, device=_dev())
    sizes = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    ins = [[rows[s][i] for s in range(S)] for i in members]
    used = dg.decompress_data_reduce(ins, [a.view for a in accs], accumulate, None, status, sizes, prob_bits=prob_bits,
                                     dtype=C.DTYPE[src.ft])
    what = f"ft={src.ft} probBits={prob_bits} S={S} accumulate={accumulate} {what}"
    assert used == 0, what
    assert status.tolist() == [1] * B, what
    assert sizes.tolist() == [src.sizes[i] for i in members], what
    want = src.expected(S, bool(accumulate))
    got = [a.bits() for a in accs]
    for k, i in enumerate(members):
        _same(got[k], C.bits(want[i]), f"{what}: member {k} ({src.sizes[i]} words)")
        assert accs[k].guards_intact(), f"{what}: member {k}: guard words overwritten"
    if sequence:
        seq = [Acc(src.sizes[i], offsets[k] if offsets else 0, fill=src.start[i] if accumulate else None) for k, i in enumerate(members)]
        for s in range(S):
            st = torch.zeros(B, dtype=torch.uint8, device=_dev())
            dg.decompress_data_accumulate([rows[s][i] for i in members], [a.view for a in seq], bool(accumulate) or s > 0, None, st,
                                          None, prob_bits=prob_bits, dtype=C.DTYPE[src.ft])
            assert st.tolist() == [1] * B, what
        for k, a in enumerate(seq):
            _same(got[k], a.bits(), f"{what}: member {k} against {S} decode-accumulate calls")


# ------------------------------------------------------------------------------------------------------ equivalence
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("prob_bits", C.PROB_BITS)
@pytest.mark.parametrize("ft", C.FTS)
def test_reduce_equals_the_sequence(ft, prob_bits, S, accumulate):
    """the staging shapes (16- and 4-block tiles, whole, ring, mixed and boundary waves, partial last blocks), every
    member with S sources whose blocks differ in kind: the numpy sequence and S decode-accumulate calls"""
    src = R.staging(ft)
    rows = _rows(src, "staging", prob_bits)
    _reduce_and_check(src, rows, S, prob_bits, list(range(len(src.sizes))), accumulate, "staging shapes", sequence=True)


# ------------------------------------------------------------------------------------------------------------ order
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("ft", C.FTS)
def test_sources_are_summed_left_to_right(ft, accumulate):
    import dietgpu_amd as dg

    hi, lo, tiny = R.ORDER_VALUES
    n = R.ORDER_WORDS
    arch = {v: _gpu(("order", ft, v), lambda v=v: _upload(O.float_compress(ft, R.constant_words(ft, v), 10))) for v in R.ORDER_VALUES}
    for order, total in (((hi, lo, tiny), 2.0 ** -10), ((tiny, hi, lo), 0.0)):
        start = np.zeros(n, np.float32)  # (+0: the sum onto it is the sum)
        a = Acc(n, fill=start if accumulate else None)
        status = torch.zeros(1, dtype=torch.uint8, device=_dev())
        dg.decompress_data_reduce([[arch[v] for v in order]], [a.view], accumulate, None, status, None, dtype=C.DTYPE[ft])
        assert status.tolist() == [1]
        want = R.reduce_expected(start, [np.full(n, v, np.float32) for v in order], bool(accumulate))
        assert (want == np.float32(total)).all()
        _same(a.bits(), C.bits(want), f"ft={ft} accumulate={accumulate} sources {order}")
        assert a.guards_intact()


# ------------------------------------------------------------------------------------------------------------ tails
@pytest.mark.parametrize("lead", [0, 3])
@pytest.mark.parametrize("ft", C.FTS)
def test_partial_last_blocks(ft, lead):
    src = R.tails(ft, lead)
    rows = _rows(src, f"tails{lead}", 10)
    members = list(range(len(src.sizes)))
    for accumulate in (0, 1):
        _reduce_and_check(src, rows, 2, 10, members, accumulate, f"lead {lead}", offsets=[i % 4 for i in members])


# -------------------------------------------------------------------------------------------- geometry and work lists
@pytest.mark.parametrize("B", [13, 67])
@pytest.mark.parametrize("ft", C.FTS)
def test_workgroup_orders_and_work_lists(ft, B):
    import dietgpu_amd as dg

    L = dg.lib()
    for tile_blocks in C.ORDER_GEOMETRIES:
        src = R.orders(ft, B, tile_blocks)
        rows = _rows(src, f"orders{B}x{tile_blocks}", 10)
        members = list(range(B))
        assert -(-max(src.sizes) // C.BLK) == C.ORDER_GEOMETRIES[tile_blocks][1]  # this geometry, two tiles per member
        for order in (0, 1, 2):
            L.dgpu_debug_set_decoder_order(order)
            try:
                for accumulate in (0, 1):
                    _reduce_and_check(src, rows, 2, 10, members, accumulate, f"order {order}, {tile_blocks}-block tiles")
            finally:
                L.dgpu_debug_set_decoder_order(-1)
        for lists in (1, 0):
            L.dgpu_debug_set_work_lists(lists)
            try:
                for accumulate in (0, 1):
                    _reduce_and_check(src, rows, 2, 10, members, accumulate, f"work lists {lists}, {tile_blocks}-block tiles")
            finally:
                L.dgpu_debug_set_work_lists(-1)


# --------------------------------------------------------------------------------------------------- all or nothing
def _failure_cases(ft, name, src):
    """-> [(what, source that is bad, (archive tensor, bytes offered), capacity of the middle member, size reported)]"""
    tile_blocks, sizes, cap1 = C.MALFORMED_BATCHES[name]
    n1 = sizes[1]
    out = []
    for s in range(3):
        good = src.archives(10)[s][1]
        for what, bad in C.corruptions(ft, good, n1, tile_blocks):
            out.append((f"source {s}: {what}", s, bad, None, cap1, n1))
        out.append((f"source {s}: truncated by 16 bytes through inBytes", s, good, good.size - 16, cap1, n1))
        # (source 0 states its own count; a later source of another count leaves source 0's)
        other = O.float_compress(ft, src.words[s][1][: n1 - 5], 10)
        out.append((f"source {s}: another word count", s, other, None, cap1, n1 - 5 if s == 0 else n1))
        other_ft = C.FTS[(C.FTS.index(ft) + 1) % 3]
        alien = O.float_compress(other_ft, C.words(other_ft, "c" * (n1 // C.BLK), n1 % C.BLK, "c", seed=4242 + s), 10)
        out.append((f"source {s}: float type {other_ft}", s, alien, None, cap1, n1))
    out.append(("capacity one word short", None, None, None, n1 - 1, n1))
    return out


@pytest.mark.parametrize("name", list(C.MALFORMED_BATCHES))
@pytest.mark.parametrize("ft", C.FTS)
def test_a_member_with_one_bad_source_keeps_every_bit(ft, name):
    """three members, three sources each; ONE source of the middle member is bad (every descriptor corruption seen from
    the first and the last tile, the pdf table, a truncated archive, another word count, another float type) or its
    capacity is a word short: status [1, 0, 1], the middle accumulator as it was, the neighbours summed"""
    import dietgpu_amd as dg

    _, sizes, _ = C.MALFORMED_BATCHES[name]
    src = R.malformed(ft, name)
    rows = _rows(src, "malformed " + name, 10)
    for what, s_bad, bad, bad_bytes, cap1, reported in _failure_cases(ft, name, src):
        ins = [[rows[s][i] for s in range(3)] for i in range(3)]
        if s_bad is not None:
            t = _upload(bad)
            ins[1][s_bad] = t[:bad_bytes] if bad_bytes is not None else t
        caps = [sizes[0], cap1, sizes[2]]
        for accumulate in (0, 1):
            # random bit patterns: finite for the neighbours, so that their sums compare bit for bit; the failing member
            # keeps ANY bits -- NaN payloads and infinities among them (copied as integers)
            fills = [R.finite_bits(cap, 10 * k + accumulate) for k, cap in enumerate(caps)]
            middle = R.any_bits(cap1, 3 + accumulate)
            assert np.isnan(middle.view(np.float32)).any()
            accs = [Acc(cap, fill=f) for cap, f in zip(caps, fills)]
            accs[1].view.view(torch.int32).copy_(torch.from_numpy(middle.view(np.int32)))
            status = torch.full((3,), 7, dtype=torch.uint8, device=_dev())
            out_sizes = torch.full((3,), -7, dtype=torch.int32, device=_dev())
            dg.decompress_data_reduce(ins, [a.view for a in accs], accumulate, None, status, out_sizes, dtype=C.DTYPE[ft])
            what2 = f"ft={ft} {name}, {what}, accumulate={accumulate}"
            assert status.tolist() == [1, 0, 1], what2
            assert out_sizes.tolist() == [sizes[0], reported, sizes[2]], what2
            _same(accs[1].bits(), middle, f"{what2}: the failing member's accumulator")
            for k in (0, 2):
                want = R.reduce_expected(fills[k], [src.wide[s][k] for s in range(3)], bool(accumulate))
                _same(accs[k].bits(), C.bits(want), f"{what2}: neighbour {k}")
            assert all(a.guards_intact() for a in accs), what2 + ": guard words overwritten"


def test_source_zero_shorter_than_a_header_reports_size_zero():
    import dietgpu_amd as dg

    src = R.malformed(C.FTS[1], "two 4-block tiles")
    rows = _rows(src, "malformed two 4-block tiles", 10)
    n = src.sizes[1]
    for short in (0, 1):  # the source that offers 8 bytes
        ins = [rows[s][1] for s in range(2)]
        ins[short] = ins[short][:8]
        fill = R.finite_bits(n, 5)
        a = Acc(n, fill=fill)
        status = torch.full((1,), 7, dtype=torch.uint8, device=_dev())
        out_sizes = torch.full((1,), -7, dtype=torch.int32, device=_dev())
        dg.decompress_data_reduce([ins], [a.view], 0, None, status, out_sizes, dtype=torch.bfloat16)
        assert status.tolist() == [0] and out_sizes.tolist() == [0 if short == 0 else n]
        _same(a.bits(), C.bits(fill), f"source {short} of 8 bytes")


# --------------------------------------------------------------------------------------------- unaligned accumulators
@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("ft", C.FTS)
def test_unaligned_accumulators(ft, offset):
    src = R.staging(ft)
    rows = _rows(src, "staging", 10)
    members = list(range(len(src.sizes)))
    for accumulate in (0, 1):
        _reduce_and_check(src, rows, 2, 10, members, accumulate, f"word offset {offset}", offsets=[offset] * len(members))


# ------------------------------------------------------------------------------------------------------------ routes
def test_routes_agree():
    import dietgpu_amd as dg

    ft, S = C.FTS[1], 3
    src = R.staging(ft)
    rows = _rows(src, "staging", 10)
    B = len(src.sizes)
    ins = [[rows[s][i] for s in range(S)] for i in range(B)]
    results = []
    try:
        for route in (False, True):
            dg.prefer_torch_ops(route)
            accs = [Acc(n, fill=src.start[i]) for i, n in enumerate(src.sizes)]
            assert dg.decompress_data_reduce(ins, [a.view for a in accs], True) == 0  # (the float type from the header)
            results.append([a.bits() for a in accs])
    finally:
        dg.prefer_torch_ops(True)
    accs = [Acc(n, fill=src.start[i]) for i, n in enumerate(src.sizes)]
    flat = [t for member in ins for t in member]
    used = ctypes.c_size_t(99)
    rc = dg.lib().dgpu_float_decode_reduce(
        None, 0, ctypes.byref(used), ft, 10, 1, B, S, (ctypes.c_void_p * (B * S))(*[r.data_ptr() for r in flat]),
        (ctypes.c_uint32 * (B * S))(*[r.numel() for r in flat]), (ctypes.c_void_p * B)(*[a.view.data_ptr() for a in accs]),
        (ctypes.c_uint32 * B)(*src.sizes), None, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and used.value == 0, dg.lib().dgpu_last_error()
    results.append([a.bits() for a in accs])
    want = src.expected(S, True)
    for k in range(B):
        for r, route in zip(results, ("ctypes", "torch op", "C ABI")):
            _same(r[k], C.bits(want[k]), f"{route}: member {k}")


# ------------------------------------------------------------------------------------------------------------- graph
def test_graph_replay_adds_the_sources_in_order():
    import dietgpu_amd as dg

    ft, S, members = C.FTS[1], 3, [0, 1, 5]
    src = R.staging(ft)
    rows = _rows(src, "staging", 10)
    ins = [[rows[s][i] for s in range(S)] for i in members]
    accs = [Acc(src.sizes[i], fill=src.start[i]) for i in members]
    views = [a.view for a in accs]
    status = torch.zeros(len(members), dtype=torch.uint8, device=_dev())

    def call():  # (dtype given: reading the header would synchronise, which a capture cannot hold)
        dg.decompress_data_reduce(ins, views, True, None, status, None, dtype=C.DTYPE[ft])

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


# --------------------------------------------------------------------------------------------------- reduce-scatter
def test_compressed_reduce_scatter_takes_the_reduce_path_rccl():
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    dietgpu_amd.lib()
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dev = _dev()
    torch.cuda.set_device(dev)
    D.init(backend="nccl", device=dev)  # "nccl" is RCCL on ROCm
    try:
        codec = D.GpuFloatCodec()
        calls = []
        inner = codec.decompress_reduce

        def spy(rows_per_acc, accs, accumulate):
            calls.append(([len(r) for r in rows_per_acc], len(accs), accumulate))
            return inner(rows_per_acc, accs, accumulate)

        codec.decompress_reduce = spy
        codec.decompress_accumulate = None  # (the loop would fail on it)
        g = torch.Generator(device="cpu").manual_seed(19)
        mine = torch.randn(100_000 + 33, generator=g).to(torch.bfloat16)
        shard, stats = D.compressed_reduce_scatter(mine.to(dev), codec=codec)
        assert calls == [([1], 1, False)]
        assert shard.dtype == torch.float32 and shard.shape == mine.shape
        assert np.array_equal(shard.cpu().numpy().view(np.uint32), C.bits(mine.to(torch.float32).numpy()))
        assert stats["payload_bytes"] < 0.75 * stats["raw_bytes"]
    finally:
        dist.destroy_process_group()
