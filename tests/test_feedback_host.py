"""Feedback cast-compress, the parts that need no GPU: the reference of the four steps (tests/feedback_ref.py) against
its literals, the exactness of the new residual against float64, the telescoping property the feature exists for, the
argument checks of the C ABI entry point (code 1 and a text, before anything touches a device) and those of the Python
layers."""
import ctypes as C

import numpy as np
import pytest
import torch

import cast_ref as R
import feedback_ref as F

A = 0x100000  # a fake device address, aligned to everything
TOO_LARGE = 1717538816 + 1
NAME = "dgpu_float_feedback_compress"
FTS = [R.BFLOAT16, R.FLOAT16]


def test_literals():
    for x, e, ft, v, q, err in F.LITERALS:
        gq, gerr, gv = F.feedback_ref([x], None if e is None else [e], ft)
        what = (hex(x), e, ft)
        assert v is None or int(gv[0]) == v, what
        assert q is None or int(gq[0]) == q, what
        assert err is None or int(gerr[0]) == err, what


def test_a_nan_leaves_a_zero_residual_whatever_the_residual_was():
    for ft in FTS:
        e = R.EDGE_BITS
        _, err, _ = F.feedback_ref(np.full(e.size, 0x7FC00000, dtype=np.uint32), e, ft)
        assert (err == 0).all()


@pytest.mark.parametrize("ft", FTS)
def test_the_new_residual_is_exact(ft):
    """float32 v - widen(q) equals the float64 difference wherever q is finite: the subtraction's rounding never shows"""
    rng = np.random.default_rng(5)
    ex, ee = np.meshgrid(R.EDGE_BITS, R.EDGE_BITS)
    x = np.concatenate([ex.ravel(), rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)])
    e = np.concatenate([ee.ravel(), rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)])
    for res in (e, None):
        q, err, v = F.feedback_ref(x, res, ft)
        w = R.widen(q, ft)
        finite = (w & 0x7F800000) != 0x7F800000
        assert finite.sum() > x.size * (0.9 if ft == R.BFLOAT16 else 0.25)  # (most random patterns overflow float16)
        exact = v.view(np.float32).astype(np.float64)[finite] - w.view(np.float32).astype(np.float64)[finite]
        assert np.array_equal(err.view(np.float32).astype(np.float64)[finite], exact)
        assert (err[~finite] == 0).all()
        # ... and it is at most half a unit in the last place of q
        assert (np.abs(exact) <= np.abs(v.view(np.float32).astype(np.float64)[finite])).all()


@pytest.mark.parametrize("ft", FTS)
def test_telescoping(ft):
    """K steps in place on a constant x: what the wire carried plus what the residual still holds is K x up to the
    rounding errors of the K adds -- per word, in float64, |sum_t widen(q_t) + e_K - K x| <= K 2^-24 max_t |v_t|"""
    rng = np.random.default_rng(9)
    n, K = 8192, 64
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 10, n))).astype(np.float32)
    if ft == R.FLOAT16:
        assert np.abs(x).max() * 2 < 65504
    e, sent, vmax = None, np.zeros(n), np.zeros(n)
    for _ in range(K):
        q, e, v = F.feedback_ref(x.view(np.uint32), e, ft)
        sent += R.widen(q, ft).view(np.float32).astype(np.float64)
        vmax = np.maximum(vmax, np.abs(v.view(np.float32).astype(np.float64)))
    left = np.abs(sent + e.view(np.float32).astype(np.float64) - K * x.astype(np.float64))
    bound = K * 2.0 ** -24 * vmax
    print("telescoping: worst left / bound", float((left / bound).max()))
    assert (left <= bound).all()
    # without feedback the same K steps lose K times one step's rounding error
    q0 = R.widen(R.cast_ref(x.view(np.uint32), ft), ft).view(np.float32).astype(np.float64)
    assert np.abs(K * q0 - K * x.astype(np.float64)).max() > 100 * left.max()


def test_entry_point_is_exported_and_bound():
    import dietgpu_amd

    raw = C.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    assert NAME in dietgpu_amd.EXPORTED_SYMBOLS and hasattr(raw, NAME)
    assert getattr(L, NAME).restype is C.c_int and len(getattr(L, NAME).argtypes) == 13
    assert callable(dietgpu_amd.compress_data_feedback)
    from dietgpu_amd import distributed

    assert callable(distributed.GpuFloatCodec.compress_cast_feedback)


def _call(n=1, floatType=2, probBits=10, inp=None, sizes=None, res_in="same", res_out=None, out=None):
    import dietgpu_amd

    L = dietgpu_amd.lib()
    used = C.c_size_t(77)
    arr = lambda v: (C.c_void_p * max(n, 1))(*v)
    sizes = sizes if sizes is not None else [4096] * n
    inp = inp if inp is not None else [A + i * 0x100000 for i in range(n)]
    res_out = res_out if res_out is not None else [A + 0x40000000 + i * 0x100000 for i in range(n)]
    out = out if out is not None else [A + 0x80000000 + i * 0x100000 for i in range(n)]
    if res_in == "same":
        res_in = res_out
    rc = getattr(L, NAME)(None, 0, C.byref(used), floatType, probBits, n, arr(inp), (C.c_uint32 * max(n, 1))(*sizes),
                          None if res_in is None else arr(res_in), None if res_out == "null" else arr(res_out), arr(out), None, None)
    return rc, L.dgpu_last_error().decode(), used.value


OVERLAP = "feedback compress: in, residualIn, residualOut and out must not overlap (residualOut[i] == residualIn[i] excepted)"
CONGRUENT = "feedback compress: in[i], residualIn[i] and residualOut[i] must be congruent modulo 16"
NULL_ENTRY = "feedback compress: null entry in a pointer array"


@pytest.mark.parametrize("over,message", [
    (dict(res_out="null", res_in=None), "feedback compress: residualOut must not be null"),
    (dict(n=2, res_out=[A + 0x40000000, 0]), NULL_ENTRY),
    (dict(n=2, res_in=[0, A + 0x50000000]), NULL_ENTRY),
    (dict(n=2, inp=[A, 0]), NULL_ENTRY),
    (dict(n=2, out=[0, A + 0x80000000]), NULL_ENTRY),
    (dict(inp=[A], res_in=[A + 0x50000004], res_out=[A + 0x40000000]), CONGRUENT),
    (dict(inp=[A], res_in=None, res_out=[A + 0x40000008]), CONGRUENT),
    (dict(inp=[A + 2], res_out=[A + 0x40000002]), "feedback compress: float32 input and residuals must be 4-byte aligned"),
    (dict(out=[A + 0x80000008]), "compressed output must be 16-byte aligned"),
    (dict(floatType=3), "floatType of a feedback archive must be float16 or bfloat16"),
    (dict(floatType=0), "floatType of a feedback archive must be float16 or bfloat16"),
    (dict(probBits=8), "probBits must be 9, 10 or 11"),
    (dict(probBits=12), "probBits must be 9, 10 or 11"),
    (dict(n=65536), "numInBatch must be <= 65535"),
    (dict(sizes=[TOO_LARGE]), "tensor larger than 1717538816 words: the maximum compressed size of its exponent plane exceeds INT32_MAX "
                              "(GpuANSEncode.cu:22)"),
    (dict(inp=[A], res_out=[A + 4096 * 4 - 16]), OVERLAP),                          # residualOut over in
    (dict(inp=[A], res_in=[A + 16], res_out=[A + 0x40000000]), OVERLAP),           # residualIn over in
    (dict(res_in=[A + 0x40000010], res_out=[A + 0x40000000]), OVERLAP),            # the residuals, shifted against each other
    (dict(n=2, res_out=[A + 0x40000000, A + 0x40000000]), OVERLAP),                # two members share a residual
    (dict(inp=[A], out=[A + 4096]), OVERLAP),                                       # the archive over in
    (dict(n=2, res_in=[A + 0x40100000, A + 0x40000000], res_out=[A + 0x40000000, A + 0x40100000]), OVERLAP),  # swapped across members
])
def test_one_fault_gives_this_code_and_text(over, message):
    rc, text, _ = _call(**over)
    assert (rc, text) == (1, message)  # DGPU_ERR_INVALID_ARGUMENT


def test_an_empty_batch_ends_after_the_checks():
    for ft in (1, 2):
        for res_in in ("same", None):
            rc, _, used = _call(n=0, floatType=ft, res_in=res_in)
            assert rc == 0 and used == 0
    # (null arrays are fine when there is nothing in them)
    rc, _, used = _call(n=0, res_out="null", res_in=None)
    assert rc == 0 and used == 0


@pytest.mark.parametrize("torch_ops", [True, False])
def test_ops_reject_bad_tensors_without_a_gpu(torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        x, r = torch.zeros(4096), torch.zeros(4096)  # CPU tensors
        with pytest.raises(RuntimeError, match="on the GPU"):
            dg.compress_data_feedback([x], [r], torch.bfloat16)
        with pytest.raises(RuntimeError):
            dg.compress_data_feedback([], [], torch.bfloat16)
        with pytest.raises(RuntimeError, match="one residual per tensor"):
            dg.compress_data_feedback([x], [], torch.bfloat16)
        with pytest.raises(RuntimeError, match="must be float32"):
            dg.compress_data_feedback([x], [r.to(torch.bfloat16)], torch.bfloat16)
        with pytest.raises(RuntimeError, match="must be float32"):
            dg.compress_data_feedback([x], [r.double()], torch.bfloat16)
        with pytest.raises(RuntimeError, match="number of elements"):
            dg.compress_data_feedback([x], [r[:4095]], torch.bfloat16)
        with pytest.raises(RuntimeError, match="must be float32"):
            dg.compress_data_feedback([x.to(torch.bfloat16)], [r], torch.bfloat16)
        for bad in (torch.float32, torch.float64, None):
            with pytest.raises(RuntimeError):
                dg.compress_data_feedback([x], [r], bad)
    finally:
        dg.prefer_torch_ops(True)


def test_collectives_reject_bad_arguments_before_any_exchange():
    from dietgpu_amd import distributed as D

    x = torch.zeros(8192)
    with pytest.raises(RuntimeError, match="raw_local"):
        D.compressed_all_reduce(x, codec=object(), wire_dtype=torch.bfloat16, raw_local=True)
    with pytest.raises(RuntimeError, match="raw_local"):
        D.compressed_reduce_scatter(x, codec=object(), wire_dtype=torch.bfloat16, raw_local=True)
    for bad in (torch.zeros(8192, dtype=torch.bfloat16), torch.zeros(8191), torch.zeros(2, 4096)[:, :4000]):
        with pytest.raises(RuntimeError, match="residual"):
            D.compressed_all_reduce(x, codec=object(), wire_dtype=torch.bfloat16, residual=bad)
    with pytest.raises(RuntimeError, match="wire_dtype"):
        D.compressed_all_reduce(x, codec=object(), wire_dtype=torch.float32)
    with pytest.raises(RuntimeError, match="wire_dtype"):
        D.compressed_all_reduce(x, codec=object(), residual=torch.zeros(8192))
    with pytest.raises(RuntimeError, match="wire_dtype"):
        D.compressed_all_reduce(x.to(torch.bfloat16), codec=object(), wire_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="compress_cast_feedback"):
        D.compressed_all_reduce(x, codec=object(), wire_dtype=torch.bfloat16, residual=torch.zeros(8192))
