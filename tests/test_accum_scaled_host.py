"""Scaled decode-accumulate, the parts that need no GPU: the arithmetic of the reference on the literals of the contract,
the premise of the GPU cases (tests/test_gpu_accum_scaled.py decodes the cases of tests/accum_cases.py at the factors of
tests/test_decode_scaled_host.py into the cases' start accumulators), the entry point being exported and bound, and the
argument errors of the C ABI and of the Python layer."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import accum_cases as C
import accum_scaled_ref as A
from test_decode_scaled_host import FACTORS, THIRD

#            type, word, factor, accumulator bits (None: accumulate off), stored float32 bits
LITERALS = [
    (A.BFLOAT16, 0x3F80, THIRD, None, 0x3EAAAAAB),
    (A.BFLOAT16, 0x3F80, THIRD, 0x3F800000, 0x3FAAAAAB),
    (A.FLOAT16, 0x3C00, -1.5, 0x3FC00000, 0x00000000),
    (A.FLOAT16, 0x0001, 1.0, None, 0x33800000),          # a float16 denormal widens to a float32 normal
    (A.BFLOAT16, 0x0000, THIRD, 0x80000000, 0x00000000),  # -0.0 + +0.0 = +0.0
    (A.BFLOAT16, 0x8000, THIRD, 0x80000000, 0x80000000),  # -0.0 + -0.0 = -0.0
    (A.BFLOAT16, 0x0080, 0.5, None, 0x00400000),          # a float32-denormal product is kept
    (A.BFLOAT16, 0x0080, 0.5, 0x00400000, 0x00800000),    # ... and added
    (A.FLOAT32, 0x00800000, 0.5, None, 0x00400000),
    (A.BFLOAT16, 0x7F7F, 2.0, None, 0x7F800000),          # the product overflows to infinity
    (A.BFLOAT16, 0x7F7F, 2.0, 0xFF7FFFFF, 0x7F800000),    # ... which the add keeps
    (A.FLOAT32, 0x7F7FFFFF, -2.0, 0x3F800000, 0xFF800000),
    (A.FLOAT16, 0x7C00, 0.5, 0x3F800000, 0x7F800000),     # acc + inf
    (A.BFLOAT16, 0x3F80, 0.0, 0x40490FDB, 0x40490FDB),    # factor 0 with accumulate: a finite accumulator keeps its bits
    (A.BFLOAT16, 0x3F80, 0.0, 0x80000000, 0x00000000),    # ... but -0 + +0 = +0
    (A.BFLOAT16, 0x3F80, 0.0, None, 0x00000000),
    (A.BFLOAT16, 0xBF80, 0.0, None, 0x80000000),
    # two roundings, not one: (1 + 2^-7) * (1 + 2^-23) rounds to 1 + 2^-7 + 2^-23 and cancels against the accumulator;
    # a fused multiply-add would leave the 2^-30 that the product's rounding drops (0x30800000)
    (A.BFLOAT16, 0x3F81, np.float32(1.0 + 2.0 ** -23), 0xBF810001, 0x00000000),
]


def test_literals():
    for ft, word, factor, acc, want in LITERALS:
        w = np.array([word], dtype=np.uint32 if ft == A.FLOAT32 else np.uint16)
        got = int(A.accum_scaled_ref(w, ft, factor, None if acc is None else np.array([acc], dtype=np.uint32))[0])
        assert got == want, f"type {ft}: {word:#x} * {float(factor)!r} + {acc}: {got:#010x}, not {want:#010x}"


def test_the_fma_literal_tells_fused_from_unfused():
    fused = np.float32(np.float64(np.float32(1.0 + 2.0 ** -7)) * np.float64(np.float32(1.0 + 2.0 ** -23))
                       + np.float64(np.array([0xBF810001], dtype=np.uint32).view(np.float32)[0]))
    assert fused.view(np.uint32) == 0x30800000  # (the float64 product and sum are exact here)


def test_nan_where_the_arithmetic_says_so():
    w = np.array([0x0000, 0x3F80, 0x7F80], dtype=np.uint16)
    assert A.is_nan(A.accum_scaled_ref(w, A.BFLOAT16, np.inf)).tolist() == [True, False, False]
    assert A.is_nan(A.accum_scaled_ref(w, A.BFLOAT16, 0.0)).tolist() == [False, False, True]
    assert A.is_nan(A.accum_scaled_ref(w, A.BFLOAT16, np.nan)).all()
    minus_inf = np.array([0xFF800000] * 3, dtype=np.uint32)
    assert A.is_nan(A.accum_scaled_ref(w, A.BFLOAT16, 1.0, minus_inf)).tolist() == [False, False, True]


@pytest.mark.parametrize("ft", C.FTS)
def test_premise_of_the_gpu_cases(ft):
    """over the cases, the factors and the cases' start accumulators no expected word is a NaN (the words, the factors
    and the accumulators are finite: a product may be an infinity, finite + infinity is an infinity): the GPU tests may
    compare every word on integer views.  The factors reach infinities and (bfloat16, float32) float32 denormals."""
    seen = {"inf": False, "denormal": False, "add changes the accumulator": False}
    for case, _ in C.all_cases(ft):
        for w, start in zip(case.words, case.start):
            assert C.finite(ft, w).all(), case.tag
            acc = C.bits(start)
            assert np.isfinite(start).all(), case.tag
            for f in FACTORS:
                p = A.accum_scaled_ref(w, ft, f)
                s = A.accum_scaled_ref(w, ft, f, acc)
                assert not A.is_nan(p).any(), f"{case.tag}: a NaN product at factor {float(f)!r}"
                assert not A.is_nan(s).any(), f"{case.tag}: a NaN sum at factor {float(f)!r}"
                mag = p & 0x7FFFFFFF
                seen["inf"] |= bool((mag == 0x7F800000).any())
                seen["denormal"] |= bool(((mag > 0) & (mag < 0x00800000)).any())
                seen["add changes the accumulator"] |= bool((s != acc).any() and (s != p).any())
    if ft == A.FLOAT16:  # (the smallest float16 times 2^-20 is a float32 normal)
        seen["denormal"] = True
    assert all(seen.values()), seen


def test_entry_point_is_exported_and_bound():
    import dietgpu_amd
    from dietgpu_amd import distributed

    name = "dgpu_float_decode_accumulate_scaled"
    raw = ctypes.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    assert name in dietgpu_amd.EXPORTED_SYMBOLS
    assert hasattr(raw, name)
    assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int
    assert L.dgpu_abi_version() == 8
    assert "scale" in inspect.signature(dietgpu_amd.decompress_data_accumulate).parameters
    assert "scale" in inspect.signature(distributed.GpuFloatCodec.decompress_accumulate).parameters
    for arg in ("out", "out_scale", "out_accumulate"):
        assert arg in inspect.signature(distributed.compressed_all_reduce).parameters
    # the op library (loaded on first use) has the op, so the torch route serves the keyword
    assert dietgpu_amd.ops._amd_op(10, "decompress_data_accumulate_scaled") is not None
    assert "Tensor? scale_dev=None" in str(torch.ops.dietgpu_amd.decompress_data_accumulate_scaled.default._schema)


def test_argument_errors_of_the_c_abi_need_no_device():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    f = L.dgpu_float_decode_accumulate_scaled
    one = (ctypes.c_uint32 * 1)(16)
    ptr = (ctypes.c_void_p * 1)(0)
    dummy = ctypes.c_void_p(4096)  # a "device" address that is never followed: every call below fails before a launch

    def fails(message, ft, P, accumulate, n, ins, in_bytes, outs, caps, scale, scale_dev, stride):
        assert f(None, 0, None, ft, P, accumulate, n, ins, in_bytes, outs, caps, scale, scale_dev, stride, None, None, None) == 1
        assert message in L.dgpu_last_error().decode(), L.dgpu_last_error().decode()

    for host in (0.5, 1.0):  # (1.0: the call forwards to decode-accumulate, whose checks are the same)
        fails("probBits must be 9, 10 or 11", 2, 12, 1, 1, ptr, one, ptr, one, host, None, 0)
        fails("probBits must be 9, 10 or 11", 2, 8, 0, 1, ptr, one, ptr, one, host, None, 0)
        fails("floatType", 0, 10, 1, 1, ptr, one, ptr, one, host, None, 0)
        fails("floatType", 4, 10, 1, 1, ptr, one, ptr, one, host, None, 0)
        fails("accumulate must be 0 or 1", 2, 10, 2, 1, ptr, one, ptr, one, host, None, 0)
        fails("accumulate must be 0 or 1", 2, 10, -1, 1, ptr, one, ptr, one, host, None, 0)
        for missing in range(4):
            arrays = [ptr, one, ptr, one]
            arrays[missing] = None
            fails("null array", 2, 10, 1, 1, *arrays, host, None, 0)
        fails("16-byte aligned", 2, 10, 1, 1, (ctypes.c_void_p * 1)(4096 + 8), one, (ctypes.c_void_p * 1)(8192), one, host, None, 0)
        fails("4-byte aligned", 2, 10, 1, 1, (ctypes.c_void_p * 1)(4096), one, (ctypes.c_void_p * 1)(8192 + 2), one, host, None, 0)
        fails("outCapacity", 2, 10, 1, 1, ptr, one, ptr, (ctypes.c_uint32 * 1)(0xfffff001), host, None, 0)
    fails("numInBatch must be <= 65535", 2, 10, 1, 65536, ptr, one, ptr, one, 0.5, None, 0)
    fails("scaleStride", 2, 10, 1, 1, ptr, one, ptr, one, 0.5, dummy, 2)
    fails("scaleStride", 2, 10, 0, 1, ptr, one, ptr, one, 0.5, None, 7)
    for bad in (0.0, -0.0, float("inf"), float("-inf"), float("nan")):
        fails("finite and not zero", 2, 10, 1, 1, ptr, one, ptr, one, bad, None, 0)
    fails("scale_dev must be 4-byte aligned", 2, 10, 1, 1, ptr, one, ptr, one, 0.5, ctypes.c_void_p(4098), 0)
    for missing in range(4):  # (a host scale is not looked at beside a device one)
        arrays = [ptr, one, ptr, one]
        arrays[missing] = None
        fails("null array", 2, 10, 1, 1, *arrays, 0.0, dummy, 1)
    for host, dev in ((0.5, None), (1.0, None), (0.0, dummy)):  # an empty batch is fine and uses nothing
        used = ctypes.c_size_t(77)
        assert f(None, 0, ctypes.byref(used), 2, 10, 1, 0, None, None, None, None, host, dev, 0, None, None, None) == 0
        assert used.value == 0


@pytest.mark.parametrize("torch_ops", [True, False])
def test_rejects_bad_arguments_without_a_gpu(torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        arch = torch.zeros(1024, dtype=torch.uint8)  # CPU tensors
        acc = torch.zeros(4096, dtype=torch.float32)
        kw = {"dtype": torch.bfloat16}
        with pytest.raises(RuntimeError):
            dg.decompress_data_accumulate([arch], [acc], True, scale=0.5, **kw)
        with pytest.raises(RuntimeError):
            dg.decompress_data_accumulate([arch], [acc], True, scale=torch.ones(1, dtype=torch.float32), **kw)
        with pytest.raises(RuntimeError):
            dg.decompress_data_accumulate([arch, arch], [acc], True, scale=0.5, **kw)
        with pytest.raises(RuntimeError):
            dg.decompress_data_accumulate([], [], True, scale=0.5, **kw)
        with pytest.raises(RuntimeError, match="float32"):  # a scale of another dtype
            dg.decompress_data_accumulate([arch], [acc], True, scale=torch.ones(1, dtype=torch.float64), **kw)
        for wrong in (0, 2, 3):  # a scale of a wrong length
            with pytest.raises(RuntimeError, match="1 element or one per archive"):
                dg.decompress_data_accumulate([arch], [acc], False, scale=torch.ones(wrong, dtype=torch.float32), **kw)
        for bad in (0.0, float("inf"), float("-inf"), float("nan"), 1e-60):  # (1e-60: its float32 is zero)
            with pytest.raises(RuntimeError, match="finite and not zero"):
                dg.decompress_data_accumulate([arch], [acc], True, scale=bad, **kw)
        with pytest.raises(RuntimeError):
            dg.decompress_data_accumulate([arch], [acc], True, scale="a third", **kw)
    finally:
        dg.prefer_torch_ops(True)
