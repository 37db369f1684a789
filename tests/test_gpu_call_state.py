"""No call depends on what temp memory or the stream held ("State shared between calls").

The per-feature tests pin every call to a host reference one feature at a time, always on fresh or library-owned temp
memory.  Here every call of tests/state_cases.py -- each C-ABI function that uses caller temp memory or the stream's
zero-at-rest counters, on the smallest case that reaches each piece of that state -- runs

  1. on temp memory of exactly its documented bound, filled with zeros, ones and random bytes, between two canaries;
  2. after every other call, on one temp buffer that is never cleared, and on the library's own slab;
  3. after each documented failure outcome;
  4. as the first call of a new stream;
  5. beside another call on a second stream, without host synchronisation;
and must leave, every time, exactly the host reference's bytes (out_sumsq: within norm_ref.check's bound, and the same 64
bits on every repeat), *tempUsed within the bound, the canaries as they were, and the stream's counters all zero
(dgpu_debug_counters_nonzero).  Tests 1 and 2 run on the ctypes route and on the torch-op route."""
import ctypes

import numpy as np
import pytest
import torch

import oracle as O
import state_cases as S

pytestmark = pytest.mark.gpu

CANARY, CANARY_BYTES = 0xC3, 4096
FILLS = ("zeros", "ones", "random")
ALL = S.ITEMS + S.FAILURES
ROUTED = [(route, item) for route in ("ctypes", "torch") for item in S.ITEMS if route == "ctypes" or item.op]
ROUTED_ALL = [(route, item) for route in ("ctypes", "torch") for item in ALL if route == "ctypes" or item.op]
_ids = lambda p: p.name if isinstance(p, S.Item) else str(p)


def _dev():
    return torch.device("cuda", 0)


def _lib():
    import dietgpu_amd as dg

    return dg.lib()


@pytest.fixture(autouse=True)
def _a_gpu_error_ends_the_module():
    """nothing more is started on a device that has reported an error"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error, no further test of this module is run: {e}", returncode=3)


@pytest.fixture
def route(request):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(request.param == "torch")
    try:
        yield request.param
    finally:
        dg.prefer_torch_ops(True)


def _counters(stream=None):
    ptr = stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return int(_lib().dgpu_debug_counters_nonzero(ctypes.c_void_p(ptr)))


def _assert_at_rest(item, what, stream=None):
    """every library-owned counter of the stream is zero; -1 (no counters yet) only after a call that makes none"""
    n = _counters(stream)
    assert n == 0 or (n == -1 and not item.counters), f"{what}: {n} of the stream's counters are not zero"


@pytest.fixture(scope="module")
def shared_temp():
    """one temp buffer of the largest bound, filled once with random bytes and never cleared"""
    need = max(item.query() for item in ALL)
    g = torch.Generator(device="cpu").manual_seed(99)
    temp = torch.randint(0, 256, (need,), dtype=torch.uint8, generator=g).to(_dev())
    return temp


# ------------------------------------------------------------------------------------------------ 1. hostile temp memory
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("route,item", ROUTED_ALL, indirect=["route"], ids=_ids)
def test_temp_memory_of_exactly_the_query_with_any_contents(route, item, fill):
    need = item.query()
    buf = torch.full((need + 2 * CANARY_BYTES,), CANARY, dtype=torch.uint8, device=_dev())
    temp = buf[CANARY_BYTES : CANARY_BYTES + need]
    assert temp.data_ptr() % 256 == 0
    if fill == "random":
        g = torch.Generator(device="cpu").manual_seed(need % 1000003)
        temp.copy_(torch.randint(0, 256, (need,), dtype=torch.uint8, generator=g))
    else:
        temp.fill_(0x00 if fill == "zeros" else 0xFF)
    what = f"{item.name}, temp memory of {need} bytes filled with {fill}, {route} route"
    outs = item.run(temp)
    item.check(outs, what)
    print(f"{item.name}: used {outs['used']} of {need} bytes ({outs['used'] / need:.4f})")
    assert 0 <= outs["used"] <= need, f"{what}: *tempUsed = {outs['used']} exceeds the documented bound {need}"
    assert bool((buf[:CANARY_BYTES] == CANARY).all()) and bool((buf[CANARY_BYTES + need :] == CANARY).all()), f"{what}: a canary was written"
    _assert_at_rest(item, what)


def test_the_decode_forms_documented_without_temp_memory_report_none(shared_temp):
    """the allow-list of tests/test_call_state_host.py: *tempUsed == 0 with temp memory on offer, once per function"""
    import dietgpu_amd as dg

    ft = O.BFLOAT16
    src, _ = S.reduce_sources("staging", ft)
    members = [1, 2]
    rows = [[torch.from_numpy(src.archives(10)[s][i].copy()).to(_dev()) for s in range(2)] for i in members]
    raw = [torch.from_numpy(src.words[1][i].view(np.int16).copy()).to(_dev()).view(torch.bfloat16) for i in members]
    accs = lambda: [torch.zeros(src.sizes[i], dtype=torch.float32, device=_dev()) for i in members]
    status = torch.zeros(2, dtype=torch.uint8, device=_dev())
    kw = dict(dtype=torch.bfloat16)
    firsts = [r[0] for r in rows]
    used = {
        "dgpu_float_decode_accumulate": dg.decompress_data_accumulate(firsts, accs(), False, shared_temp, status, None, **kw),
        "dgpu_float_decode_accumulate_scaled": dg.decompress_data_accumulate(firsts, accs(), False, shared_temp, status, None, scale=S.THIRD, **kw),
        "dgpu_float_decode_reduce": dg.decompress_data_reduce(rows, accs(), False, shared_temp, status, None, **kw),
        "dgpu_float_decode_reduce_mixed": dg.decompress_data_reduce_mixed([[r[0], w] for r, w in zip(rows, raw)], accs(), False, shared_temp, status, None, **kw),
        "dgpu_float_decode_reduce_scaled": dg.decompress_data_reduce(rows, accs(), False, shared_temp, status, None, scale=S.THIRD, **kw),
        "dgpu_float_decode_scaled": dg.decompress_data_scaled(firsts, [torch.zeros(src.sizes[i], dtype=torch.bfloat16, device=_dev()) for i in members],
                                                             S.THIRD, shared_temp, status, None),
        "dgpu_float_decompress_range": dg.decompress_data_range(True, firsts, [torch.zeros(S.BLK, dtype=torch.bfloat16, device=_dev()) for _ in members],
                                                                [0, 1], [1, 1], shared_temp, status, None),
    }
    x = torch.from_numpy(O.ans_encode(S.case_bytes("pairs")[2], 10)).to(_dev())
    used["dgpu_ans_decode_batch_pointer_range"] = dg.decompress_data_range(False, [x], [torch.zeros(S.BLK, dtype=torch.uint8, device=_dev())], [0], [1],
                                                                           shared_temp, status[:1], None)
    torch.cuda.synchronize()
    assert set(used) == set(S.NO_TEMP)
    assert all(v == 0 for v in used.values()), used
    assert bool(status.all())


# --------------------------------------------------------------------------------------------------- 2. every ordered pair
@pytest.mark.parametrize("route,first", ROUTED, indirect=["route"], ids=_ids)
def test_every_call_after_this_one_on_temp_memory_that_is_never_cleared(route, first, shared_temp):
    followers = [item for r, item in ROUTED if r == route]
    for temp, where in ((shared_temp, "the shared temp buffer"), (None, "the library's slab")):
        first.check(first.run(temp), f"{first.name} on {where}, {route} route")
        _assert_at_rest(first, first.name)
        for k, item in enumerate(followers):
            if k:
                first.run(temp)  # (checked above and in its own turn as a follower: here it only leaves its state behind)
            what = f"{item.name} after {first.name} on {where}, {route} route"
            item.check(item.run(temp), what)
            _assert_at_rest(item, what)


# ------------------------------------------------------------------------------------------------------ 3. after a failure
@pytest.mark.parametrize("failure", S.FAILURES, ids=_ids)
def test_every_call_after_a_documented_failure(failure, shared_temp):
    for item in S.ITEMS:
        what = f"{failure.name}, before {item.name}"
        failure.check(failure.run(shared_temp), what)
        _assert_at_rest(failure, what)
        what = f"{item.name} after {failure.name}"
        item.check(item.run(shared_temp), what)
        _assert_at_rest(item, what)


# ----------------------------------------------------------------------------------------------------------- 4. a new stream
@pytest.mark.parametrize("item", S.ITEMS, ids=_ids)
def test_the_first_two_calls_of_a_new_stream(item):
    item.prepare()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    try:
        repeats = []
        for call in range(2):
            what = f"{item.name}, call {call} of a new stream"
            outs = item.run(None, stream)
            stream.synchronize()
            item.check(outs, what)
            # a stream of its own: the counters exist exactly when this call uses them
            assert _counters(stream) == (0 if item.counters else -1), f"{what}: dgpu_debug_counters_nonzero = {_counters(stream)}"
            if hasattr(item, "repeatable"):
                repeats.append(item.repeatable(outs))
        assert not repeats or repeats[0] == repeats[1], f"{item.name}: the norm outputs of two identical calls differ in their bits"
    finally:
        torch.cuda.synchronize()
        released = _lib().dgpu_release_stream_state(ctypes.c_void_p(stream.cuda_stream))
        assert released == 1, released
    assert _counters(stream) == -1  # (the state is gone, and asking has not made a new one)


# ------------------------------------------------------------------------------------------------------------ 5. two streams
_PAIRED = ("reduce-compress-plain/staging", "float-compress-bfloat16/pairs", "float-compress-bfloat16/large")


@pytest.mark.parametrize("a,b", [(_PAIRED[0], _PAIRED[1]), (_PAIRED[1], _PAIRED[2]), (_PAIRED[2], _PAIRED[0])])
def test_two_streams_side_by_side_without_host_synchronisation(a, b):
    a, b = S.BY_NAME[a], S.BY_NAME[b]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    temps = [torch.full((item.query(),), 0xFF, dtype=torch.uint8, device=_dev()) for item in (a, b)]
    for item in (a, b):
        item.prepare()
    torch.cuda.synchronize()
    try:
        outs = []
        for _ in range(4):
            outs.append((a, a.run(temps[0], streams[0])))
            outs.append((b, b.run(temps[1], streams[1])))
        torch.cuda.synchronize()  # the only one
        for k, (item, o) in enumerate(outs):
            item.check(o, f"{item.name}, round {k // 2}, beside {(b if item is a else a).name} on another stream")
        for item, stream in zip((a, b), streams):
            _assert_at_rest(item, f"{item.name} on its own stream after four rounds", stream)
            assert _counters(stream) == 0
    finally:
        torch.cuda.synchronize()
        for stream in streams:
            _lib().dgpu_release_stream_state(ctypes.c_void_p(stream.cuda_stream))
