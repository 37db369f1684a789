"""k_ans_decode_accum on the paths that N(0, 1) inputs never reach: both staging modes for every float type (and waves
that mix them, and blocks at the 1024-word limit), partial last blocks on both sides of every 8-row group, every
workgroup order, capacities larger than the element, accumulators that are rows of one matrix, malformed descriptors
seen from every tile, two streams.

The inputs are the cases of tests/accum_cases.py, whose premises tests/test_accumulate_cases_host.py asserts with the
CPU oracle; the archives are the oracle's.  Every expected value is built on the host from the input words -- the exact
widening (torch on the CPU) and numpy float32 adds -- and compared BIT FOR BIT on uint32 views, every word of it."""
import ctypes

import numpy as np
import pytest
import torch

import accum_cases as C
from test_gpu_accumulate import GUARD, SENTINEL, Acc, _dev

pytestmark = pytest.mark.gpu

SENTINEL2 = np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0]  # capacity past the element's end
_rows_cache = {}


def _rows(case, prob_bits):
    """the case's oracle archives on the GPU, uploaded once"""
    key = (case.tag, case.ft, prob_bits)
    if key not in _rows_cache:
        _rows_cache[key] = [torch.from_numpy(a.copy()).to(_dev()) for a in case.archives(prob_bits)]
    return _rows_cache[key]


def _want(case, i, accumulate):
    return C.bits(case.sums(1)[i] if accumulate else case.wide[i])


def _same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} words differ, the first at {bad[:4].tolist()}"


def _decode_batch(case, prob_bits, members, accumulate, what, offsets=None):
    """one call for `members` of the case: status, sizes, every accumulator word and the guards"""
    import dietgpu_amd as dg

    rows = _rows(case, prob_bits)
    B = len(members)
    accs = [Acc(case.sizes[i], offsets[k] if offsets else 0, fill=case.start[i] if accumulate else None)
            for k, i in enumerate(members)]
    status = torch.full((B,), 7, dtype=torch.uint8, device=_dev())
    sizes = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    used = dg.decompress_data_accumulate([rows[i] for i in members], [a.view for a in accs], accumulate, None, status, sizes,
                                         prob_bits=prob_bits)
    what = f"{case.tag} ft={case.ft} probBits={prob_bits} accumulate={accumulate} {what}"
    assert used == 0, what
    assert status.tolist() == [1] * B, what
    assert sizes.tolist() == [case.sizes[i] for i in members], what
    for k, (i, a) in enumerate(zip(members, accs)):
        _same(a.bits(), _want(case, i, accumulate), f"{what}: member {k} ({case.sizes[i]} words)")
        assert a.guards_intact(), f"{what}: member {k} ({case.sizes[i]} words): guard words overwritten"


# ------------------------------------------------------------------------------------------------ 1. staging modes
@pytest.mark.parametrize("prob_bits", C.PROB_BITS)
@pytest.mark.parametrize("ft", C.FTS)
def test_staging_modes_in_one_call(ft, prob_bits):
    """whole-staged, ring, mixed and boundary waves, 16-block and 4-block tiles: each element alone, then all together"""
    case = C.staging(ft, 0)
    everything = list(range(len(case.sizes)))
    for members in [[i] for i in everything] + [everything]:
        for accumulate in (False, True):
            _decode_batch(case, prob_bits, members, accumulate, f"members {members}")


# ---------------------------------------------------------------------------------------- 2. partial last blocks
@pytest.mark.parametrize("lead", C.LEADS)
@pytest.mark.parametrize("ft", C.FTS)
def test_partial_last_blocks_at_every_row_count(ft, lead):
    """last blocks of 1 .. 4095 words on both sides of the 8-row group boundaries, behind 0, 1, 3 or 8 whole blocks,
    compressible (staged whole) and incompressible (ring) by turns, accumulators at every word offset"""
    case = C.tails(ft, lead)
    members = list(range(len(case.sizes)))
    for accumulate in (False, True):
        _decode_batch(case, 10, members, accumulate, f"lead {lead}", offsets=[i % 4 for i in members])


# ------------------------------------------------------------------------------------------- 3. workgroup orders
@pytest.mark.parametrize("B", C.ORDER_BATCHES)
@pytest.mark.parametrize("ft", C.FTS)
def test_workgroup_orders(ft, B):
    """element-major, tile-major and per-XCD order (the library picks the last for B >= 64, its grid padded to a multiple
    of 8 elements), then the work list forced on and off: batches whose rectangle is full enough to be launched as one"""
    import dietgpu_amd as dg

    L = dg.lib()
    for tile_blocks in C.ORDER_GEOMETRIES:
        case = C.orders(ft, B, tile_blocks)
        members = list(range(B))
        assert -(-max(case.sizes) // C.BLK) == C.ORDER_GEOMETRIES[tile_blocks][1]  # this geometry
        tiles = C.tiles_of(case.sizes, tile_blocks)
        assert min(tiles) >= 2 and 5 * sum(tiles) > 4 * B * max(tiles)  # the policy keeps the rectangle
        for order in (-1, 0, 1, 2):
            L.dgpu_debug_set_decoder_order(order)
            try:
                for accumulate in (False, True):
                    _decode_batch(case, 10, members, accumulate, f"order {order}, {tile_blocks}-block tiles")
            finally:
                L.dgpu_debug_set_decoder_order(-1)
        if B == max(C.ORDER_BATCHES):
            for lists in (1, 0):
                L.dgpu_debug_set_work_lists(lists)
                try:
                    for accumulate in (False, True):
                        _decode_batch(case, 10, members, accumulate, f"work lists {lists}, {tile_blocks}-block tiles")
                finally:
                    L.dgpu_debug_set_work_lists(-1)


# ------------------------------------------------------------------------------ 4. capacity larger than the element
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
    batches += [(everything, [rules[(i + 1) % len(rules)][1](n) for i, n in enumerate(case.sizes)], "all, assorted capacities")]
    for members, caps, what in batches:
        assert all(cap > case.sizes[i] for i, cap in zip(members, caps))
        for accumulate in (False, True):
            accs = [Acc(cap) for cap in caps]
            for i, a in zip(members, accs):
                a.view[case.sizes[i]:].view(torch.int32).fill_(int(SENTINEL2))
                if accumulate:
                    a.view[: case.sizes[i]].copy_(torch.from_numpy(case.start[i]))
            status = torch.full((len(members),), 7, dtype=torch.uint8, device=_dev())
            sizes = torch.full((len(members),), -7, dtype=torch.int32, device=_dev())
            dg.decompress_data_accumulate([rows[i] for i in members], [a.view for a in accs], accumulate, None, status, sizes)
            what2 = f"ft={ft} accumulate={accumulate} {what}"
            assert status.tolist() == [1] * len(members), what2
            assert sizes.tolist() == [case.sizes[i] for i in members], what2
            for i, a in zip(members, accs):
                got, n = a.bits(), case.sizes[i]
                _same(got[:n], _want(case, i, accumulate), f"{what2}: element {i}")
                assert (got[n:].view(np.int32) == SENTINEL2).all(), f"{what2}: element {i}: words past its size were written"
                assert a.guards_intact(), f"{what2}: element {i}: guard words overwritten"


# --------------------------------------------------------------------------------- 5. accumulators as matrix rows
def _call(route, ft, accumulate, ins, outs, status, sizes):
    """decode-accumulate at probBits 10 through the torch op, the ctypes binding or the bare C ABI"""
    import dietgpu_amd as dg

    if route == "cabi":
        B = len(ins)
        used = ctypes.c_size_t(99)
        rc = dg.lib().dgpu_float_decode_accumulate(
            None, 0, ctypes.byref(used), ft, 10, int(accumulate), B, (ctypes.c_void_p * B)(*[r.data_ptr() for r in ins]),
            (ctypes.c_uint32 * B)(*[r.numel() for r in ins]), (ctypes.c_void_p * B)(*[o.data_ptr() for o in outs]),
            (ctypes.c_uint32 * B)(*[o.numel() for o in outs]), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(sizes.data_ptr()),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0 and used.value == 0, dg.lib().dgpu_last_error()
        return
    dg.prefer_torch_ops(route == "torch_ops")
    try:
        assert dg.decompress_data_accumulate(ins, outs, accumulate, None, status, sizes, prob_bits=10) == 0
    finally:
        dg.prefer_torch_ops(True)


@pytest.mark.parametrize("route", ["torch_ops", "ctypes", "cabi"])
@pytest.mark.parametrize("ft", C.FTS)
def test_accumulators_as_rows_of_one_matrix(ft, route):
    """equal capacities at addresses in arithmetic progression, ascending or descending, are passed as a stride; the
    same rows scrambled as a pointer list.  Rows outside the call are not touched."""
    case = C.rows(ft)
    rows = _rows(case, 10)
    n = C.ROW_WORDS
    for order in C.ROW_ORDERS:
        for accumulate in (False, True):
            buf = torch.full((2 * GUARD + 6 * n,), int(SENTINEL), dtype=torch.int32, device=_dev())
            mat = buf[GUARD : GUARD + 6 * n].view(torch.float32).view(6, n)
            if accumulate:
                mat.copy_(torch.from_numpy(np.stack(case.start)))
            status = torch.full((len(order),), 7, dtype=torch.uint8, device=_dev())
            sizes = torch.full((len(order),), -7, dtype=torch.int32, device=_dev())
            _call(route, ft, accumulate, [rows[i] for i in order], [mat[i] for i in order], status, sizes)
            what = f"ft={ft} {route} rows {order} accumulate={accumulate}"
            assert status.tolist() == [1] * len(order) and sizes.tolist() == [n] * len(order), what
            got = buf.cpu().numpy()
            assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + 6 * n :] == SENTINEL).all(), what + ": guard words overwritten"
            got = got[GUARD : GUARD + 6 * n].view(np.uint32).reshape(6, n)
            for i in range(6):
                if i in order:
                    _same(got[i], _want(case, i, accumulate), f"{what}: row {i}")
                else:
                    untouched = C.bits(case.start[i]) if accumulate else np.full(n, SENTINEL, np.int32).view(np.uint32)
                    _same(got[i], untouched, f"{what}: row {i}, which is not in the call")


# -------------------------------------------------------------------------------------- 6. malformed descriptors
@pytest.mark.parametrize("name", list(C.MALFORMED_BATCHES))
@pytest.mark.parametrize("ft", C.FTS)
def test_a_malformed_element_stores_nothing_from_any_tile(ft, name):
    """every tile checks every block descriptor and the pdf table: a bad descriptor in the first tile stops the last
    tile, one in the last tile stops the first, and the neighbours in the batch are summed as if nothing had happened"""
    import dietgpu_amd as dg

    tile_blocks, sizes, cap1 = C.MALFORMED_BATCHES[name]
    case = C.malformed(ft, name)
    rows = _rows(case, 10)
    caps = [sizes[0], cap1, sizes[2]]
    assert -(-max(caps) // C.BLK) > tile_blocks and (tile_blocks == 16) == (max(caps) > 8 * C.BLK)
    fill1 = np.concatenate([case.start[1], C.random_acc(cap1 - sizes[1], 61)])
    for what, bad in C.corruptions(ft, case.archives(10)[1], sizes[1], tile_blocks):
        ins = [rows[0], torch.from_numpy(bad).to(_dev()), rows[2]]
        for accumulate in (False, True):
            fills = [case.start[0], fill1, case.start[2]] if accumulate else [None] * 3
            accs = [Acc(cap, fill=f) for cap, f in zip(caps, fills)]
            status = torch.full((3,), 7, dtype=torch.uint8, device=_dev())
            out_sizes = torch.full((3,), -7, dtype=torch.int32, device=_dev())
            dg.decompress_data_accumulate(ins, [a.view for a in accs], accumulate, None, status, out_sizes)
            what2 = f"ft={ft} {name}, {what}, accumulate={accumulate}"
            assert status.tolist() == [1, 0, 1], what2
            assert out_sizes.tolist() == sizes, what2  # the header is valid in every case
            before = C.bits(fill1) if accumulate else np.full(cap1, SENTINEL, np.int32).view(np.uint32)
            _same(accs[1].bits(), before, f"{what2}: the failing member's accumulator")
            for k in (0, 2):
                _same(accs[k].bits(), _want(case, k, accumulate), f"{what2}: neighbour {k}")
            assert all(a.guards_intact() for a in accs), what2 + ": guard words overwritten"


# ------------------------------------------------------------------------------------------------- 7. two streams
@pytest.mark.parametrize("ft", C.FTS)
def test_two_streams_accumulate_concurrently(ft):
    """two different batches of staging elements, three accumulating calls each on their own stream and into their own
    accumulators, no host synchronisation in between: three successive float32 adds per word"""
    import dietgpu_amd as dg

    cases = [C.staging(ft, 0), C.staging(ft, 1)]
    reps = 3
    rows = [_rows(c, 10) for c in cases]
    accs = [[Acc(n, fill=s) for n, s in zip(c.sizes, c.start)] for c in cases]
    status = [[torch.full((len(c.sizes),), 7, dtype=torch.uint8, device=_dev()) for _ in range(reps)] for c in cases]
    streams = [torch.cuda.Stream(device=_dev()) for _ in cases]
    torch.cuda.synchronize()
    for rep in range(reps):
        for k, st in enumerate(streams):
            with torch.cuda.stream(st):
                dg.decompress_data_accumulate(rows[k], [a.view for a in accs[k]], True, None, status[k][rep], None,
                                              dtype=C.DTYPE[ft])
    torch.cuda.synchronize()
    for k, c in enumerate(cases):
        assert all(s.tolist() == [1] * len(c.sizes) for s in status[k]), f"stream {k}"
        for i, a in enumerate(accs[k]):
            _same(a.bits(), C.bits(c.sums(reps)[i]), f"ft={ft} stream {k}, element {i} ({c.sizes[i]} words)")
            assert a.guards_intact(), f"stream {k}, element {i}: guard words overwritten"
