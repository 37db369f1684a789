"""dgpu_float_rolling_compress on the GPU: the table of a call from the counts of the last one, the counts of a call taken
by the encoder while it codes.  Archives are compared BYTE FOR BYTE with tests/rolling_ref.py (the CPU oracle's float
archive under the smoothed counts) and, where the counts are the data's own, with the plain call's; counts with
np.bincount of the exponent bytes.  Every output is poisoned first; a guard row lies behind the archives and another
behind the counts, and both are looked at after every call."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import cast_ref
import oracle as O
import rolling_ref as R

pytestmark = pytest.mark.gpu

BLK = 4096
FTS = [R.BFLOAT16, R.FLOAT16]
_TORCH = {R.BFLOAT16: torch.bfloat16, R.FLOAT16: torch.float16}
POISON = 0xA5
SIZES = [1, 31, 4095, 4096, 4097, 2 * BLK + 33, 4 * BLK, 5 * BLK + 1, 8 * BLK, 17 * BLK + 100, 40 * BLK + 4095]


def _dev():
    return torch.device("cuda:0")


def _bits(n, seed, scale=1.0):
    """float32 bits: N(0, scale^2) with the edge patterns of tests/cast_ref.py (NaN, inf, denormals, ties) among them"""
    rng = np.random.default_rng(seed)
    b = (rng.standard_normal(n) * scale).astype(np.float32).view(np.uint32).copy()
    k = min(n, cast_ref.EDGE_BITS.size)
    b[rng.choice(n, k, replace=False)] = cast_ref.EDGE_BITS[:k]
    return b


def _upload16(words, ft):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int16).copy()).to(_dev()).view(_TORCH[ft])


def _upload32(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int32).copy()).to(_dev()).view(torch.float32)


class Counts:
    """[n, 256] int32 on the GPU with a guard row behind it"""

    def __init__(self, n, fill=None):
        self.n = n
        self.buf = torch.full((n + 1, 256), -0x5A5A5A5B, dtype=torch.int32, device=_dev())
        if fill is not None:
            self.buf[:n].copy_(torch.from_numpy(np.ascontiguousarray(fill).astype(np.uint32).view(np.int32).reshape(n, 256)))
        self.t = self.buf[:n]

    def host(self):
        assert bool((self.buf[self.n] == -0x5A5A5A5B).all()), "the guard row behind the counts was written"
        return self.t.cpu().numpy().view(np.uint32)


def _call(ts, cin, cout, ft, cast, prob_bits=10, cap=None, temp=None, out=None, fetch=None):
    """-> (archives as numpy arrays up to min(size, cap) -- of the members `fetch`, default all --, sizes, temp bytes
    used, comp matrix)"""
    import dietgpu_amd as dg

    n = len(ts)
    if cap is None:
        cap = int(dg.lib().dgpu_float_max_compressed_size(ft, max(t.numel() for t in ts)))
    if out is None:
        comp = torch.full((n + 1, cap), POISON, dtype=torch.uint8, device=_dev())
        sizes = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    else:
        comp, sizes = out
    got, gsz, used = dg.compress_data_rolling(ts, None if cin is None else cin.t, None if cout is None else cout.t,
                                              _TORCH[ft] if cast else None, temp, comp, sizes, prob_bits=prob_bits)
    torch.cuda.synchronize()
    assert got.data_ptr() == comp.data_ptr()
    assert bool((comp[n] == POISON).all()), "the guard row behind the archives was written"
    host_sizes = sizes.cpu().numpy().view(np.uint32).tolist()
    archives = {i: comp[i, : min(host_sizes[i], cap)].cpu().numpy() for i in (range(n) if fetch is None else fetch)}
    return archives, host_sizes, used, comp


def _same(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, "first differing byte", int(bad[0]), "of", want.size)


def _decode(comp, ts, ft, words, prob_bits=10):
    import dietgpu_amd as dg

    outs = [torch.zeros(t.numel(), dtype=_TORCH[ft], device=_dev()) for t in ts]
    status = torch.zeros(len(ts), dtype=torch.uint8, device=_dev())
    dg.decompress_data(True, [comp[i] for i in range(len(ts))], outs, False, None, status, None, prob_bits=prob_bits)
    torch.cuda.synchronize()
    assert bool(status.all())
    for o, w in zip(outs, words):
        assert (o.view(torch.int16).cpu().numpy().view(np.uint16) == w).all()


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("cast", [False, True])
@pytest.mark.parametrize("prob_bits", [9, 10, 11])
@pytest.mark.parametrize("ft", FTS)
def test_counts_only_leaves_the_plain_archive_and_exact_counts(ft, prob_bits, cast):
    import dietgpu_amd as dg

    bits = [_bits(n, 100 * ft + n % 97) for n in SIZES]
    words = [cast_ref.cast_ref(b, ft) for b in bits]
    ts = [_upload32(b) for b in bits] if cast else [_upload16(w, ft) for w in words]
    cout = Counts(len(ts))
    got, sizes, used, _ = _call(ts, None, cout, ft, cast, prob_bits)
    assert 0 < used <= int(dg.lib().dgpu_float_compress_temp_bytes(ft, len(ts), max(SIZES)))
    plain, psz, _ = (dg.compress_data_cast(ts, _TORCH[ft], prob_bits=prob_bits) if cast
                     else dg.compress_data(True, ts, False, prob_bits=prob_bits))
    torch.cuda.synchronize()
    counts = cout.host()
    for i, w in enumerate(words):
        want = O.float_compress(ft, w, prob_bits)
        assert sizes[i] == want.size == int(psz[i])
        _same(got[i], want, f"element {i} ({w.size} words) against the oracle")
        _same(got[i], plain[i, : sizes[i]].cpu().numpy(), f"element {i} against the plain call")
        assert (counts[i] == R.exponent_hist(ft, w)).all(), (i, w.size)
        assert int(counts[i].sum()) == w.size


def test_an_empty_element_gets_zero_counts_and_its_header():
    ts = [torch.empty(0, dtype=torch.bfloat16, device=_dev()), _upload16(cast_ref.cast_ref(_bits(5000, 1), R.BFLOAT16), R.BFLOAT16)]
    c = Counts(2)
    got, sizes, _, _ = _call(ts, None, c, R.BFLOAT16, False)
    assert (c.host()[0] == 0).all() and int(c.host()[1].sum()) == 5000
    _same(got[0], O.float_compress(R.BFLOAT16, np.zeros(0, np.uint16), 10), "empty element")
    got2, _, _, _ = _call(ts, c, c, R.BFLOAT16, False)
    assert (c.host()[0] == 0).all() and int(c.host()[1].sum()) == 5000
    _same(got2[0], got[0], "empty element, rolling")
    w = cast_ref.cast_ref(_bits(5000, 1), R.BFLOAT16)
    _same(got2[1], R.expected_archive(R.BFLOAT16, w, 10, R.smooth(R.exponent_hist(R.BFLOAT16, w), 5000)), "own counts, smoothed")


# ------------------------------------------------------------------------------------------------------------ 2
def _step_inputs(ft, n, seed):
    """x0 ~ N(0, 1), x1 ~ 3 N(0, 1) with a few exponents x0 lacks"""
    x0 = cast_ref.cast_ref(_bits(n, seed)[: n], ft)
    b1 = _bits(n, seed + 1, 3.0)
    b1[:: max(n // 7, 1)] = np.array([0x7E000000, 0x00800000, 0x5F000000, 0x10000000, 0x447A0000, 0x46EA6000, 0xC4FA0000, 0x461C4000],
                                     np.uint32)[: len(b1[:: max(n // 7, 1)])]
    return x0, cast_ref.cast_ref(b1, ft), b1


@pytest.mark.parametrize("torch_ops", [True, False])
@pytest.mark.parametrize("cast", [False, True])
@pytest.mark.parametrize("ft", FTS)
def test_one_rolling_step(ft, cast, torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        sizes = [9 * BLK + 7, 3 * BLK, 777]
        x0, x1, b1 = zip(*[_step_inputs(ft, n, 10 * ft + i) for i, n in enumerate(sizes)])
        assert all((R.exponent_hist(ft, b)[R.exponent_hist(ft, a) == 0] > 0).any() for a, b in zip(x0[:2], x1[:2]))
        up = (lambda w: _upload32(cast_ref.widen(w, ft))) if cast else (lambda w: _upload16(w, ft))
        c = Counts(len(sizes))
        _call([up(w) for w in x0], None, c, ft, cast)
        assert all((c.host()[i] == R.exponent_hist(ft, w)).all() for i, w in enumerate(x0))
        t1 = [_upload32(b) for b in b1] if cast else [_upload16(w, ft) for w in x1]
        got, gsz, _, comp = _call(t1, c, c, ft, cast)  # aliased: one buffer, which now holds x1's counts
        for i, w in enumerate(x1):
            want = R.expected_archive(ft, w, 10, R.smooth(R.exponent_hist(ft, x0[i]), w.size))
            assert gsz[i] == want.size
            _same(got[i], want, f"element {i}")
            assert (c.host()[i] == R.exponent_hist(ft, w)).all()
        _decode(comp, t1, ft, x1)
    finally:
        dg.prefer_torch_ops(True)


# ------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("prob_bits", [9, 10, 11])
@pytest.mark.parametrize("ft", FTS)
def test_counts_that_cover_nothing(ft, prob_bits):
    """the spill path at prob_bits bits per symbol: no element fails, whatever the counts buffer holds"""
    n = 9 * BLK + 7
    w = np.random.default_rng(prob_bits + ft).integers(0, 1 << 16, n, dtype=np.uint16)
    ts = [_upload16(w, ft)]
    for counts in (R.exponent_hist(ft, np.zeros(n, np.uint16)), np.zeros(256, np.uint32), np.full(256, 0xFFFFFFFF, np.uint32)):
        cin, cout = Counts(1, counts), Counts(1)
        got, gsz, _, comp = _call(ts, cin, cout, ft, False, prob_bits)
        want = R.expected_archive(ft, w, prob_bits, R.smooth(counts, n))
        assert gsz[0] == want.size == R.sizes_blockwise(ft, w, prob_bits, R.smooth(counts, n))
        _same(got[0], want, "hostile counts")
        assert (cin.host()[0] == counts).all() and (cout.host()[0] == R.exponent_hist(ft, w)).all()
        _decode(comp, ts, ft, [w], prob_bits)


@pytest.mark.parametrize("blocks,dispatch", [(1, -1), (2, 1), (2, 0), (4, 1), (4, 0)])
@pytest.mark.parametrize("ft", FTS)
def test_counts_that_cover_nothing_on_the_plain_small_tile_encoders(ft, blocks, dispatch):
    """counts_in without counts_out runs the PLAIN encoders of every form: k_ans_encode_pair for a batch of single-block
    elements (the table comes from the pdf in the header), 2- and 4-block tiles persistent (0) and hardware-dispatched (1),
    whose wavefronts all take a spill-slot pair out of the pool here: P 11, random bit patterns, counts of zeros."""
    import dietgpu_amd as dg

    P, B = 11, 300
    rng = np.random.default_rng(31 * blocks + ft)
    sizes = [int(rng.integers(1, blocks * BLK + 1)) for _ in range(B)]
    sizes[:4] = [blocks * BLK, 1, max(blocks * BLK - 1, 1), (blocks - 1) * BLK + 1]
    ws = [rng.integers(0, 1 << 16, n, dtype=np.uint16) for n in sizes]
    ts = [_upload16(w, ft) for w in ws]
    hostile = np.stack([R.exponent_hist(ft, np.zeros(n, np.uint16)) for n in sizes])
    cin = Counts(B, hostile)
    L = dg.lib()
    L.dgpu_debug_set_encoder_dispatch(dispatch)
    try:
        got, gsz, _, comp = _call(ts, cin, None, ft, False, P)
    finally:
        L.dgpu_debug_set_encoder_dispatch(-1)
    assert (cin.host() == hostile).all()
    for i, w in enumerate(ws):
        want = R.expected_archive(ft, w, P, R.smooth(hostile[i], w.size))
        assert gsz[i] == want.size, (i, w.size)
        _same(got[i], want, f"member {i} ({w.size} words)")
    _decode(comp, ts, ft, ws, P)


# ------------------------------------------------------------------------------------------------------------ 4
def _geometry_members():
    rng = np.random.default_rng(4)
    blocks = [1 + (i * 7) % 40 for i in range(67)]
    return [b * BLK - int(rng.integers(0, 4095)) for b in blocks]


@pytest.fixture(scope="module")
def geometry_reference():
    ft = R.BFLOAT16
    sizes = _geometry_members()
    x0 = [cast_ref.cast_ref(_bits(n, 400 + i), ft) for i, n in enumerate(sizes)]
    x1 = [cast_ref.cast_ref(_bits(n, 900 + i, 2.0), ft) for i, n in enumerate(sizes)]
    a0 = [O.float_compress(ft, w, 10) for w in x0]
    a1 = [R.expected_archive(ft, w, 10, R.smooth(R.exponent_hist(ft, v), w.size)) for w, v in zip(x1, x0)]
    return x0, x1, a0, a1


@pytest.mark.parametrize("mode", [1, 0])
def test_work_lists_and_size_classes(geometry_reference, mode):
    import dietgpu_amd as dg

    ft = R.BFLOAT16
    x0, x1, a0, a1 = geometry_reference
    L = dg.lib()
    L.dgpu_debug_set_work_lists(mode)
    L.dgpu_debug_set_size_classes(mode)
    try:
        c = Counts(len(x0))
        got, _, _, _ = _call([_upload16(w, ft) for w in x0], None, c, ft, False)
        for i, w in enumerate(x0):
            _same(got[i], a0[i], f"counting, member {i}")
            assert (c.host()[i] == R.exponent_hist(ft, w)).all(), i
        t1 = [_upload16(w, ft) for w in x1]
        got, _, _, comp = _call(t1, c, c, ft, False)
        for i, w in enumerate(x1):
            _same(got[i], a1[i], f"rolling, member {i}")
            assert (c.host()[i] == R.exponent_hist(ft, w)).all(), i
    finally:
        L.dgpu_debug_set_work_lists(-1)
        L.dgpu_debug_set_size_classes(-1)


# ------------------------------------------------------------------------------------------------------------ 5
def test_more_tiles_than_resident_workgroups():
    import dietgpu_amd as dg

    ft, B, n = R.BFLOAT16, 4000, 2 * BLK
    g = torch.Generator(device=_dev()).manual_seed(5)
    m0 = torch.randn((B, n), generator=g, device=_dev()).to(torch.bfloat16)
    m1 = (torch.randn((B, n), generator=g, device=_dev()) * 2.5).to(torch.bfloat16)

    def hist(m):
        e = ((m.view(torch.int16).to(torch.int32) >> 7) & 0xFF) + 256 * torch.arange(B, device=_dev(), dtype=torch.int32)[:, None]
        return torch.bincount(e.reshape(-1).to(torch.int64), minlength=256 * B).reshape(B, 256).cpu().numpy().astype(np.uint32)

    c = Counts(B)
    _call([m0[i] for i in range(B)], None, c, ft, False, fetch=[])
    h0 = hist(m0)
    assert (c.host() == h0).all()
    t1 = [m1[i] for i in range(B)]
    got, gsz, _, comp = _call(t1, c, c, ft, False, fetch=range(0, B, 97))
    assert (c.host() == hist(m1)).all()
    w1 = m1.view(torch.int16).cpu().numpy().view(np.uint16)
    for i in range(0, B, 97):
        _same(got[i], R.expected_archive(ft, w1[i], 10, R.smooth(h0[i], n)), f"member {i}")
    outs = torch.zeros_like(m1)
    status = torch.zeros(B, dtype=torch.uint8, device=_dev())
    dg.decompress_data(True, [comp[i] for i in range(B)], [outs[i] for i in range(B)], False, None, status, None)
    torch.cuda.synchronize()
    assert bool(status.all()) and torch.equal(outs.view(torch.int16), m1.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------ 6
def test_stolen_tiles_are_counted_once():
    import dietgpu_amd as dg

    ft = R.BFLOAT16
    x0 = [cast_ref.cast_ref(_bits(40 * BLK, 60 + i), ft) for i in range(8)]
    x1 = [cast_ref.cast_ref(_bits(40 * BLK, 70 + i, 1.5), ft) for i in range(8)]
    t0, t1 = [_upload16(w, ft) for w in x0], [_upload16(w, ft) for w in x1]

    def run():
        c = Counts(8)
        a, _, _, _ = _call(t0, None, c, ft, False)
        h = c.host().copy()
        b, _, _, _ = _call(t1, c, c, ft, False)
        return a, h, b, c.host().copy()

    plain = run()
    L = dg.lib()
    L.dgpu_debug_set_absent_workgroups(3)
    try:
        hooked = run()
    finally:
        L.dgpu_debug_set_absent_workgroups(0)
    for i in range(8):
        assert (hooked[1][i] == R.exponent_hist(ft, x0[i])).all() and (hooked[3][i] == R.exponent_hist(ft, x1[i])).all()
        _same(hooked[0][i], plain[0][i], f"counting, member {i}")
        _same(hooked[2][i], plain[2][i], f"rolling, member {i}")
    _same(plain[0][0], O.float_compress(ft, x0[0], 10), "member 0 against the oracle")


# ------------------------------------------------------------------------------------------------------------ 7
def test_an_archive_beyond_the_maximum_is_clipped_and_reported():
    import dietgpu_amd as dg

    ft, P = R.BFLOAT16, 11
    hostile = R.exponent_hist(ft, np.zeros(8, np.uint16)) * 1000000
    rng = np.random.default_rng(7)
    full = rng.integers(0, 1 << 16, 905 * BLK, dtype=np.uint16)
    chosen = None
    for blocks in range(890, 906):  # the reference alone decides which size crosses the maximum by a little
        n = blocks * BLK - 5
        over = R.sizes_blockwise(ft, full[:n], P, R.smooth(hostile, n)) - O.float_max_compressed_size(ft, n)
        if 16 <= over <= 4096:
            chosen = (n, over)
            break
    assert chosen is not None
    n, over = chosen
    w = full[:n]
    cap = O.float_max_compressed_size(ft, n)
    assert cap == int(dg.lib().dgpu_float_max_compressed_size(ft, n))
    want = R.expected_archive(ft, w, P, R.smooth(hostile, n))
    assert want.size == cap + over
    cin = Counts(1, hostile)
    got, gsz, _, _ = _call([_upload16(w, ft)], cin, None, ft, False, P, cap=cap)  # (the guard row lies right behind `cap`)
    assert gsz[0] == cap + over, (gsz[0], cap, over)
    _same(got[0], want[:cap], "the first max bytes")


# ------------------------------------------------------------------------------------------------------------ 8
def test_no_histogram_kernel_runs_with_counts_in():
    import dietgpu_amd as dg

    ft = R.BFLOAT16
    L = dg.lib()
    ws = [cast_ref.cast_ref(_bits(n, n), ft) for n in (12 * BLK + 1, 3 * BLK, 100)]
    ts = [_upload16(w, ft) for w in ws]
    c = Counts(3)

    def profiled(cin):
        L.dgpu_prof_reset()
        L.dgpu_prof_enable(1)
        try:
            _call(ts, cin, c, ft, False)
        finally:
            L.dgpu_prof_enable(0)
        buf = C.create_string_buffer(8192)
        assert L.dgpu_prof_summary(buf, 8192) > 0
        L.dgpu_prof_reset()
        return json.loads(buf.value.decode())

    first = profiled(None)
    assert any(k.startswith("k_float_histogram") for k in first), first
    assert first["k_ans_encode_count"]["launches"] == 1 and "k_normalize" not in first
    steady = profiled(c)
    assert not any(k.startswith("k_float_histogram") or k.startswith("k_histogram") or k == "k_stats_single" for k in steady), steady
    assert steady["k_normalize"]["launches"] == 1 and steady["k_ans_encode_count"]["launches"] == 1
    assert set(steady) == {"k_normalize", "k_ans_encode_count"}, steady


# ------------------------------------------------------------------------------------------------------------ 9
def test_an_aliased_rolling_call_replays_in_a_hip_graph():
    import dietgpu_amd as dg

    ft, sizes = R.BFLOAT16, [9 * BLK + 7, 2 * BLK, 4097]
    xs = [torch.zeros(n, dtype=torch.bfloat16, device=_dev()) for n in sizes]
    cap = int(dg.lib().dgpu_float_max_compressed_size(ft, max(sizes)))
    comp = torch.full((len(sizes) + 1, cap), POISON, dtype=torch.uint8, device=_dev())
    out_sizes = torch.zeros(len(sizes), dtype=torch.int32, device=_dev())
    temp = torch.empty((int(dg.lib().dgpu_float_compress_temp_bytes(ft, len(sizes), max(sizes))),), dtype=torch.uint8, device=_dev())
    c = Counts(len(sizes))

    def fresh(step):
        return [cast_ref.cast_ref(_bits(n, 1000 + 10 * step + i, 1.0 + 0.5 * step), ft) for i, n in enumerate(sizes)]

    def load(words):
        for x, w in zip(xs, words):
            x.copy_(_upload16(w, ft))

    prev = fresh(0)
    load(prev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dg.compress_data_rolling(xs, None, c.t, None, temp, comp, out_sizes)  # leaves the counts of step 0
        dg.compress_data_rolling(xs, c.t, c.t, None, temp, comp, out_sizes)   # the warm call, identical to the captured one
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        dg.compress_data_rolling(xs, c.t, c.t, None, temp, comp, out_sizes)
    torch.cuda.synchronize()
    for step in range(1, 4):
        cur = fresh(step)
        load(cur)
        comp.fill_(POISON)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert bool((comp[len(sizes)] == POISON).all())
        got_sizes = out_sizes.cpu().tolist()
        for i, w in enumerate(cur):
            want = R.expected_archive(ft, w, 10, R.smooth(R.exponent_hist(ft, prev[i]), w.size))
            assert got_sizes[i] == want.size
            _same(comp[i, : want.size].cpu().numpy(), want, f"replay {step}, element {i}")
            assert (c.host()[i] == R.exponent_hist(ft, w)).all()
        prev = cur
