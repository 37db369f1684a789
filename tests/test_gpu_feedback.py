"""dgpu_float_feedback_compress on the GPU: float32 tensors and their float32 residuals in, ordinary bfloat16 / float16
archives and the new residuals out.  The reference of the archive is the library's own compress_data_cast of v = x + e
(tests/feedback_ref.py) uploaded as a float32 tensor -- that call is pinned to the oracle by tests/test_gpu_cast.py --
compared byte for byte; the reference of the residual is feedback_ref, compared bit for bit.  Every residual buffer
sits between guard words that must keep their pattern, and the inputs must come back unchanged."""
import ctypes

import numpy as np
import pytest
import torch

import cast_ref as R
import feedback_ref as F

pytestmark = pytest.mark.gpu

BLK = 4096
FTS = [R.BFLOAT16, R.FLOAT16]
_TORCH = {R.BFLOAT16: torch.bfloat16, R.FLOAT16: torch.float16}
SIZES = [1, 7, 8, 9, 255, 256, 257, 4095, 4096, 4097, 2 * BLK + 5, 4 * BLK - 1, 4 * BLK + 300, 8 * BLK + 1, 17 * BLK + 250]
GUARD = 64  # words in front of and behind every residual buffer (256 bytes: the buffer keeps its alignment)
PATTERN = 0x5A5A1234
QNAN = 0x7FC00000


def _dev():
    return torch.device("cuda:0")


def _normal_bits(n, seed):
    """N(0, 1) * 2^k with k changing every few thousand words: compressible exponents over a wide range"""
    rng = np.random.default_rng(seed)
    k = rng.integers(-30, 30, n // 3000 + 1).repeat(3000)[:n]
    return (rng.standard_normal(n) * np.exp2(k)).astype(np.float32).view(np.uint32)


def _random_bits(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _to_dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint32).view(np.int32).copy()).to(_dev())


def _bits_of(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


class Guarded:
    """n float32 words `off` words past a 16-byte boundary, GUARD pattern words on either side"""

    def __init__(self, n, off, bits=None, fill=PATTERN):
        self.n, self.start = n, GUARD + off
        self.buf = torch.full((GUARD + off + n + GUARD,), PATTERN, dtype=torch.int32, device=_dev())
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[self.start : self.start + n].view(torch.float32)
        if bits is not None:
            self.t.view(torch.int32).copy_(_to_dev(bits))
        elif fill != PATTERN:
            self.t.view(torch.int32).fill_(fill)

    def check_guards(self, what):
        assert bool((self.buf[: self.start] == PATTERN).all()) and bool((self.buf[self.start + self.n :] == PATTERN).all()), \
            f"{what}: words outside the residual were written"

    def bits(self):
        return _bits_of(self.t)


class Case:
    """float32 elements x (host bits) with their residuals e (host bits; None: no residual yet) at word offsets `offs`"""

    def __init__(self, x_bits, e_bits, offs=None):
        self.x = [np.ascontiguousarray(b, dtype=np.uint32) for b in x_bits]
        self.e = None if e_bits is None else [np.ascontiguousarray(b, dtype=np.uint32) for b in e_bits]
        self.offs = offs or [0] * len(self.x)
        self.tx = [Guarded(b.size, o, b) for b, o in zip(self.x, self.offs)]
        self._want = {}

    def sub(self, members):
        c = Case.__new__(Case)
        c.x, c.offs, c.tx = [self.x[i] for i in members], [self.offs[i] for i in members], [self.tx[i] for i in members]
        c.e = None if self.e is None else [self.e[i] for i in members]
        c._want = {}
        return c

    def residuals(self, fill=None):
        """fresh guarded residual buffers holding e (fill: that pattern instead)"""
        if fill is not None or self.e is None:
            return [Guarded(b.size, o, fill=QNAN if fill is None else fill) for b, o in zip(self.x, self.offs)]
        return [Guarded(b.size, o, e) for b, o, e in zip(self.x, self.offs, self.e)]

    def ref(self, ft):
        """-> per member (q, e', v)"""
        return [F.feedback_ref(x, None if self.e is None else self.e[i], ft) for i, x in enumerate(self.x)]

    def want(self, ft, prob_bits=10):
        """-> (archives of v by compress_data_cast [B, cap], their sizes, the new residual bits per member)"""
        import dietgpu_amd as dg

        key = (ft, prob_bits)
        if key not in self._want:
            ref = self.ref(ft)
            tv = [Guarded(v.size, o, v).t for (_, _, v), o in zip(ref, self.offs)]
            comp, sizes, _ = dg.compress_data_cast(tv, _TORCH[ft], prob_bits=prob_bits)
            torch.cuda.synchronize()
            self._want[key] = (comp, sizes.tolist(), [r[1] for r in ref])
        return self._want[key]

    def same(self, comp, sizes, res, ft, prob_bits, what):
        want, want_sizes, want_res = self.want(ft, prob_bits)
        what = f"ft={ft} probBits={prob_bits} {what}"
        B = len(self.x)
        assert sizes[:B].tolist() == want_sizes, what
        cap = want.shape[1]
        mask = torch.arange(cap, device=_dev())[None, :] < torch.tensor(want_sizes, device=_dev())[:, None]
        zero = torch.zeros_like(want)
        if not torch.equal(torch.where(mask, comp[:B, :cap], zero), torch.where(mask, want, zero)):
            got, w = comp.cpu().numpy(), want.cpu().numpy()
            for i, n in enumerate(want_sizes):
                bad = np.nonzero(got[i, :n] != w[i, :n])[0]
                assert bad.size == 0, f"{what}: member {i} ({self.x[i].size} words): {bad.size} archive bytes differ, the first at {bad[:4].tolist()}"
        for i, (g, w) in enumerate(zip(res, want_res)):
            got = g.bits()
            bad = np.nonzero(got != w)[0]
            assert bad.size == 0, (f"{what}: member {i} ({self.x[i].size} words at offset {self.offs[i]}): {bad.size} residual words differ, the "
                                   f"first at {bad[:4].tolist()}: got {[hex(v) for v in got[bad[:4]]]} want {[hex(v) for v in w[bad[:4]]]}")
            g.check_guards(f"{what}: member {i}")

    def unchanged(self):
        for g, b in zip(self.tx, self.x):
            assert np.array_equal(g.bits(), b), "the input was modified"
            g.check_guards("input")

    def run(self, ft, what, prob_bits=10, **kw):
        """one in-place call through dietgpu_amd.ops from the case's residual, checked against the reference"""
        import dietgpu_amd as dg

        res = self.residuals()
        comp, sizes, _ = dg.compress_data_feedback([g.t for g in self.tx], [g.t for g in res], _TORCH[ft], self.e is None, prob_bits=prob_bits, **kw)
        self.same(comp, sizes, res, ft, prob_bits, what)
        return comp, sizes, res


_cache = {}


def _cached(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def _first_step_residual(n, seed, ft=R.BFLOAT16):
    """what a first feedback step leaves of another N(0, 1) * 2^k tensor: realistic magnitudes"""
    return F.feedback_ref(_normal_bits(n, seed), None, ft)[1]


def _mixed():
    """the sizes of the contract; x N(0, 1) * 2^k and random bit patterns by turns; e a first step's residual, for two
    members random bit patterns; sources at every word offset"""
    def make():
        xs = [(_normal_bits if i % 3 else _random_bits)(n, 100 + i) for i, n in enumerate(SIZES)]
        es = [_first_step_residual(n, 300 + i) for i, n in enumerate(SIZES)]
        for i in (6, 13):
            es[i] = F.unambiguous(xs[i], _random_bits(SIZES[i], 400 + i))
        return Case(xs, es, [i % 4 for i in range(len(SIZES))])
    return _cached("mixed", make)


def _classes300():
    """300 members of 3 size classes (2-, 4- and 8-block tiles; the single-block members run on the 2-block tiles)"""
    def make():
        sizes = [300 + i % 7 if i % 3 == 0 else ((2 * BLK + 100 + i % 7) if i % 3 == 1 else (4 * BLK + 9 + i % 7)) for i in range(300)]
        xs = [(_normal_bits if i % 5 else _random_bits)(n, 500 + i) for i, n in enumerate(sizes)]
        es = [F.unambiguous(x, _first_step_residual(x.size, 900 + i)) for i, x in enumerate(xs)]
        return Case(xs, es)
    return _cached("classes300", make)


# -------------------------------------------------------------------------------------------------------- 1. edge table
ROT = 7  # EDGE_BITS rotated by 7 meets no NaN with a NaN and no infinity with the opposite one
EDGE_X = R.EDGE_BITS
EDGE_E = np.roll(R.EDGE_BITS, -ROT)


def test_the_rotation_is_unambiguous():
    assert np.array_equal(F.unambiguous(EDGE_X, EDGE_E), EDGE_E)


@pytest.mark.parametrize("ft", FTS)
def test_edge_table_on_the_vector_path(ft):
    """every edge of add, rounding and residual in an element of 3 blocks + 37 words: full-block chunks, and again in
    the last, partial block"""
    n = EDGE_X.size
    x = np.concatenate([np.resize(EDGE_X, 2 * BLK), _normal_bits(BLK - n, 1), EDGE_X, EDGE_X[:37]])
    e = np.concatenate([np.resize(EDGE_E, 2 * BLK), _first_step_residual(BLK - n, 2), EDGE_E, EDGE_E[:37]])
    assert x.size == 3 * BLK + 37
    c = Case([x], [e])
    c.run(ft, "edge table, vector path")
    c.unchanged()
    Case([x], None).run(ft, "edge table, vector path, no residual yet")


@pytest.mark.parametrize("ft", FTS)
def test_edge_table_in_the_last_slice_and_as_three_word_elements(ft):
    """the same pairs three at a time: as the last, partial 16-byte slice of a 43-word element and as 3-word elements,
    at byte offsets 0 (aligned windows, tail form) and 4 (the load that ends at the last byte; the scalar path)"""
    xs, es, offs = [], [], []
    for i in range(0, EDGE_X.size, 3):
        x3, e3 = np.resize(EDGE_X[i : i + 3], 3), np.resize(EDGE_E[i : i + 3], 3)
        for off in (0, 1):
            xs += [np.concatenate([_normal_bits(40, i), x3]), x3]
            es += [np.concatenate([_first_step_residual(40, i + 1), e3]), e3]
            offs += [off, off]
    c = Case(xs, es, offs)
    c.run(ft, "edge table, last slice and 3-word elements")
    c.unchanged()
    Case(xs, None, offs).run(ft, "edge table, last slice and 3-word elements, no residual yet")


# --------------------------------------------------------------------------------------------------------------- 2. sizes
@pytest.mark.parametrize("ft", FTS)
def test_sizes_one_member_at_a_time_and_as_one_batch(ft):
    c = _mixed()
    for i in range(len(SIZES)):
        c.sub([i]).run(ft, f"size {SIZES[i]} alone")
    c.run(ft, "mixed batch")
    c.unchanged()


# ------------------------------------------------------------------------------------- 3. three uses of the residual pointers
def _cabi(case, ft, prob_bits, res_in, res_out):
    """the C ABI called directly, with the temp region its contract names -> (comp, sizes, tempUsed, contract)"""
    import dietgpu_amd as dg

    L = dg.lib()
    B = len(case.x)
    mx = max(b.size for b in case.x)
    cap = int(L.dgpu_float_max_compressed_size(ft, mx))
    contract = int(L.dgpu_float_compress_temp_bytes(ft, B, mx))
    temp = torch.empty((contract,), dtype=torch.uint8, device=_dev())
    comp = torch.zeros((B, cap), dtype=torch.uint8, device=_dev())
    sizes = torch.zeros((B,), dtype=torch.int32, device=_dev())
    used = ctypes.c_size_t(0)
    ptrs = lambda ts: (ctypes.c_void_p * B)(*[t.data_ptr() for t in ts])
    rc = L.dgpu_float_feedback_compress(
        ctypes.c_void_p(temp.data_ptr()), contract, ctypes.byref(used), ft, prob_bits, B, ptrs([g.t for g in case.tx]),
        (ctypes.c_uint32 * B)(*[b.size for b in case.x]), None if res_in is None else ptrs([g.t for g in res_in]), ptrs([g.t for g in res_out]),
        (ctypes.c_void_p * B)(*[comp.data_ptr() + i * cap for i in range(B)]), ctypes.c_void_p(sizes.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.dgpu_last_error().decode()
    torch.cuda.synchronize()
    return comp, sizes, int(used.value), contract


@pytest.mark.parametrize("ft", FTS)
def test_in_place_and_out_of_place_leave_the_same_bits(ft):
    c = _mixed()
    res_in, res_out = c.residuals(), c.residuals(fill=PATTERN)
    comp, sizes, _, _ = _cabi(c, ft, 10, res_in, res_out)
    c.same(comp, sizes, res_out, ft, 10, "out of place")
    for g, e in zip(res_in, c.e):
        assert np.array_equal(g.bits(), e), "residualIn was written by an out-of-place call"
        g.check_guards("residualIn")
    comp2, sizes2, _, _ = _cabi(c, ft, 10, res_in, res_in)
    c.same(comp2, sizes2, res_in, ft, 10, "in place")
    c.unchanged()


@pytest.mark.parametrize("ft", FTS)
def test_fresh_ignores_what_the_buffer_holds(ft):
    """no residual yet: the archive is compress_data_cast(x) whatever the buffer held (NaNs here), -0 keeps its sign"""
    import dietgpu_amd as dg

    c = _mixed()
    fresh = Case.__new__(Case)
    fresh.x, fresh.e, fresh.offs, fresh.tx, fresh._want = c.x, None, c.offs, c.tx, {}
    res = fresh.residuals(fill=QNAN)
    comp, sizes, _ = dg.compress_data_feedback([g.t for g in fresh.tx], [g.t for g in res], _TORCH[ft], True)
    fresh.same(comp, sizes, res, ft, 10, "fresh")
    plain, psizes, _ = dg.compress_data_cast([g.t for g in fresh.tx], _TORCH[ft])
    assert psizes.tolist() == sizes.tolist()
    for i, n in enumerate(sizes.tolist()):
        assert torch.equal(comp[i, :n], plain[i, :n]), f"member {i}: the archive of a fresh step is not compress_data_cast's"
    z = Case([np.full(5, 0x80000000, dtype=np.uint32), np.full(BLK + 3, 0x80000000, dtype=np.uint32)], None, [1, 0])
    _, _, zres = z.run(ft, "-0, no residual yet")
    assert all((g.bits() == 0).all() for g in zres)


@pytest.mark.parametrize("ft", FTS)
def test_four_steps_in_place_with_a_changing_x(ft):
    import dietgpu_amd as dg

    sizes = [2 * BLK + 5, 43, 8 * BLK + 1]
    offs = [0, 3, 2]
    res, e = None, None
    for step in range(4):
        c = Case([_normal_bits(n, 40 + 10 * step + i) for i, n in enumerate(sizes)], e, offs)
        if res is None:
            res = c.residuals()
        comp, csz, _ = dg.compress_data_feedback([g.t for g in c.tx], [g.t for g in res], _TORCH[ft], step == 0)
        c.same(comp, csz, res, ft, 10, f"step {step}")
        e = c.want(ft)[2]


# ------------------------------------------------------------------------------------------------------- 4. every offset
@pytest.mark.parametrize("ft", FTS)
def test_every_offset_of_the_pair(ft):
    sizes = [3, 43, BLK + 300, 8 * BLK + 1]
    xs = [_normal_bits(n, 20 + off) for off in range(4) for n in sizes]
    es = [_first_step_residual(n, 60 + off) for off in range(4) for n in sizes]
    c = Case(xs, es, [off for off in range(4) for _ in sizes])
    assert sorted({g.t.data_ptr() % 16 for g in c.tx}) == [0, 4, 8, 12]
    for i in range(len(xs)):
        c.sub([i]).run(ft, f"{xs[i].size} words at byte offset {4 * c.offs[i]}")
    c.run(ft, "all offsets in one batch")
    c.unchanged()


# -------------------------------------------------------------------------------------------------------- 5. host routes
@pytest.mark.parametrize("which", ["mixed", "classes300"])
@pytest.mark.parametrize("ft", FTS)
def test_forced_host_routes(ft, which):
    """both encoder dispatch forms, work lists on and off, size classes on, off and under the policy, parameter cache on
    and off; in place each time from the same starting residual: archives and residuals do not depend on the route"""
    import dietgpu_amd as dg

    L = dg.lib()
    c = _mixed() if which == "mixed" else _classes300()
    c.want(ft)
    try:
        for dispatch in (0, 1):
            for lists in (0, 1):
                for classes in (-1, 0, 1):
                    for cache in (1, 0):
                        L.dgpu_debug_set_encoder_dispatch(dispatch)
                        L.dgpu_debug_set_work_lists(lists)
                        L.dgpu_debug_set_size_classes(classes)
                        L.dgpu_debug_set_param_cache(cache)
                        c.run(ft, f"{which}: dispatch {dispatch} work lists {lists} size classes {classes} parameter cache {cache}")
    finally:
        L.dgpu_debug_set_encoder_dispatch(-1)
        L.dgpu_debug_set_work_lists(-1)
        L.dgpu_debug_set_size_classes(-1)
        L.dgpu_debug_set_param_cache(1)
    c.unchanged()


@pytest.mark.parametrize("ft", FTS)
def test_a_tile_that_is_taken_over_updates_each_word_once(ft):
    """workgroups that start late: their tiles are encoded by the workgroups that need them; in place, every residual word
    is still read once and written once"""
    import dietgpu_amd as dg

    L = dg.lib()
    c = _mixed()
    c.want(ft)
    try:
        L.dgpu_debug_set_absent_workgroups(3)
        for dispatch in (0, 1):
            L.dgpu_debug_set_encoder_dispatch(dispatch)
            c.run(ft, f"absent workgroups, dispatch {dispatch}")
    finally:
        L.dgpu_debug_set_absent_workgroups(0)
        L.dgpu_debug_set_encoder_dispatch(-1)


# -------------------------------------------------------------------------------------------------- 6. precision and routes
@pytest.mark.parametrize("prob_bits", [9, 10, 11])
@pytest.mark.parametrize("ft", FTS)
def test_prob_bits_on_the_c_abi_and_the_temp_contract(ft, prob_bits):
    c = _mixed()
    res = c.residuals()
    comp, sizes, used, contract = _cabi(c, ft, prob_bits, res, res)
    c.same(comp, sizes, res, ft, prob_bits, "C ABI, mixed batch")
    assert 0 < used <= contract, (used, contract)
    for members in ([0], [3], [14]):  # the smallest, a single-block and the largest member alone
        s = c.sub(members)
        res = s.residuals()
        comp, sizes, used, contract = _cabi(s, ft, prob_bits, res, res)
        s.same(comp, sizes, res, ft, prob_bits, f"C ABI, member {members}")
        assert 0 < used <= contract, (used, contract)


@pytest.mark.parametrize("torch_ops", [True, False])
@pytest.mark.parametrize("ft", FTS)
def test_op_route_and_ctypes_route(ft, torch_ops):
    import dietgpu_amd as dg

    c = _mixed()
    dg.prefer_torch_ops(torch_ops)
    try:
        c.run(ft, f"torch_ops={torch_ops}")
        # caller's output tensors and temp memory, as compress_data takes them
        want = c.want(ft)[0]
        B = len(c.x)
        out = torch.zeros((B + 1, want.shape[1] + 16), dtype=torch.uint8, device=_dev())
        osz = torch.zeros((B + 1,), dtype=torch.int32, device=_dev())
        temp = torch.empty((int(dg.lib().dgpu_float_compress_temp_bytes(ft, B, max(SIZES))),), dtype=torch.uint8, device=_dev())
        res = c.residuals()
        comp, sizes, used = dg.compress_data_feedback([g.t for g in c.tx], [g.t for g in res], _TORCH[ft], False, temp, out, osz)
        assert comp.data_ptr() == out.data_ptr() and sizes.data_ptr() == osz.data_ptr() and 0 < used <= temp.numel()
        c.same(comp, sizes, res, ft, 10, f"torch_ops={torch_ops}, caller's outputs")
    finally:
        dg.prefer_torch_ops(True)


class _View:
    """a tensor that is a view of somebody else's storage, with Guarded's reading interface"""

    def __init__(self, t):
        self.t = t

    def bits(self):
        return _bits_of(self.t)

    def check_guards(self, what):
        pass


@pytest.mark.parametrize("ft", FTS)
def test_rows_of_two_matrices_of_an_odd_width(ft):
    """x the rows of one matrix, the residual the rows of a second one: arithmetic progressions of 4-byte aligned
    addresses on all three pointer arrays (stride views), then the same rows in a scrambled order (an uploaded list)"""
    import dietgpu_amd as dg

    rows, width = 12, 2 * BLK + 301
    xb = _normal_bits(rows * width, 30).reshape(rows, width)
    eb = _first_step_residual(rows * width, 31).reshape(rows, width)
    mx = _to_dev(xb.reshape(-1)).view(torch.float32).view(rows, width)
    for order in (list(range(rows)), [7, 2, 11, 0, 5, 9, 1, 10, 3, 8, 6, 4]):
        me = _to_dev(eb.reshape(-1)).view(torch.float32).view(rows, width)
        c = Case.__new__(Case)
        c.x, c.e, c.offs, c.tx, c._want = [xb[i] for i in order], [eb[i] for i in order], [0] * rows, [_View(mx[i]) for i in order], {}
        comp, sizes, _ = dg.compress_data_feedback([mx[i] for i in order], [me[i] for i in order], _TORCH[ft])
        c.same(comp, sizes, [_View(me[i]) for i in order], ft, 10, f"matrix rows in order {order}")
    assert np.array_equal(_bits_of(mx).reshape(rows, width), xb)


# --------------------------------------------------------------------------------------------------------- 7. graph capture
def test_an_in_place_call_replays_in_a_hip_graph():
    """captured after one identical warm call on a side stream (a single branch): two replays advance the in-place residual
    two steps and leave the second step's archive"""
    import dietgpu_amd as dg

    ft, sizes, offs = R.BFLOAT16, [9 * BLK + 7, 2 * BLK, 4097], [0, 1, 2]
    c0 = Case([_normal_bits(n, 70 + i) for i, n in enumerate(sizes)], [_first_step_residual(n, 80 + i) for i, n in enumerate(sizes)], offs)
    xs = [g.t for g in c0.tx]
    res = c0.residuals()
    rs = [g.t for g in res]
    cap = int(dg.lib().dgpu_float_max_compressed_size(ft, max(sizes)))
    comp = torch.zeros((len(sizes), cap), dtype=torch.uint8, device=_dev())
    out_sizes = torch.zeros((len(sizes),), dtype=torch.int32, device=_dev())
    temp = torch.empty((int(dg.lib().dgpu_float_compress_temp_bytes(ft, len(sizes), max(sizes))),), dtype=torch.uint8, device=_dev())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dg.compress_data_feedback(xs, rs, _TORCH[ft], False, temp, comp, out_sizes)  # the warm call, identical to the captured one
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        dg.compress_data_feedback(xs, rs, _TORCH[ft], False, temp, comp, out_sizes)
    torch.cuda.synchronize()
    # back to the starting residual; then two replays = two steps
    for g, e in zip(res, c0.e):
        g.t.view(torch.int32).copy_(_to_dev(e))
    torch.cuda.synchronize()
    e1 = c0.want(ft)[2]
    c1 = Case.__new__(Case)
    c1.x, c1.e, c1.offs, c1.tx, c1._want = c0.x, e1, offs, c0.tx, {}
    c1.want(ft)
    comp.zero_()
    torch.cuda.synchronize()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    c1.same(comp, out_sizes, res, ft, 10, "after two replays")
    c0.unchanged()
    del graph
    dg.lib().dgpu_release_graph_state()


# ------------------------------------------------------------------------------------------------------------ 8. round trip
@pytest.mark.parametrize("ft", FTS)
def test_round_trip_gives_q(ft):
    import dietgpu_amd as dg

    c = _mixed()
    comp, sizes, _ = c.run(ft, "round trip")
    rows = [comp[i, :n] for i, n in enumerate(sizes.tolist())]
    outs = [torch.empty((x.size,), dtype=_TORCH[ft], device=_dev()) for x in c.x]
    status = torch.zeros((len(rows),), dtype=torch.uint8, device=_dev())
    dg.decompress_data(True, rows, outs, False, None, status, None)
    assert status.tolist() == [1] * len(rows)
    for i, (q, _, _) in enumerate(c.ref(ft)):
        assert np.array_equal(outs[i].view(torch.int16).cpu().numpy().view(np.uint16), q), f"member {i}: decoded words"
