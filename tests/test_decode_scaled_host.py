"""Scaled decompress, the parts that need no GPU: the arithmetic of the reference on the literals of the contract, the
premises of the GPU cases (tests/test_gpu_decode_scaled.py decodes the cases of tests/accum_cases.py at these factors),
the entry point being exported and bound, and the argument errors of the C ABI and of the Python layer."""
import ctypes

import numpy as np
import pytest
import torch

import accum_cases as C
import scaled_ref as S

THIRD = np.float32(1.0 / 3.0)
FACTORS = (THIRD, np.float32(-1.5), np.float32(2.0 ** -20), np.float32(3.0e38))

#            type, word, factor, stored
LITERALS = [
    (S.BFLOAT16, 0x3F80, THIRD, 0x3EAB),
    (S.BFLOAT16, 0xC040, -1.5, 0x4090),
    (S.BFLOAT16, 0x7F7F, 2.0, 0x7F80),
    (S.BFLOAT16, 0x0080, 0.5, 0x0040),  # a float32 denormal kept
    (S.BFLOAT16, 0x0001, 0.5, 0x0000),  # tie to even
    (S.BFLOAT16, 0x8000, THIRD, 0x8000),
    (S.FLOAT16, 0x3C00, THIRD, 0x3555),
    (S.FLOAT16, 0x7BFF, 2.0, 0x7C00),
    (S.FLOAT16, 0x0400, 0.5, 0x0200),
    (S.FLOAT16, 0x0001, 0.5, 0x0000),
    (S.FLOAT16, 0x0003, 0.5, 0x0002),
    (S.FLOAT16, 0x3C00, 2.0 ** -25, 0x0000),
    (S.FLOAT16, 0x3C01, 2.0 ** -25, 0x0001),
    (S.FLOAT16, 0x4248, 2.0 ** -20, 0x0032),
    (S.FLOAT16, 0x7C00, -1.0, 0xFC00),
]


def test_literals():
    for ft, word, factor, want in LITERALS:
        got = int(S.scaled_ref(np.array([word], dtype=np.uint16), ft, factor)[0])
        assert got == want, f"type {ft}: {word:#06x} * {float(factor)!r} -> {got:#06x}, not {want:#06x}"


def test_reference_special_factors():
    for ft, one, zero, nzero, inf in ((S.BFLOAT16, 0x3F80, 0x0000, 0x8000, 0x7F80), (S.FLOAT16, 0x3C00, 0x0000, 0x8000, 0x7C00)):
        w = np.array([one, one | 0x8000, zero, nzero, inf], dtype=np.uint16)
        assert S.scaled_ref(w, ft, 0.0)[:4].tolist() == [zero, nzero, zero, nzero]
        assert S.is_nan(S.scaled_ref(w, ft, 0.0), ft).tolist() == [False] * 4 + [True]
        by_inf = S.scaled_ref(w, ft, np.inf)
        assert by_inf[:2].tolist() == [inf, inf | 0x8000] and by_inf[4] == inf
        assert S.is_nan(by_inf, ft).tolist() == [False, False, True, True, False]
        assert np.array_equal(S.scaled_ref(w, ft, 1.0), w)
    w = np.array([0x3F800000, 0x00000001, 0x7F800000], dtype=np.uint32)
    assert S.scaled_ref(w, S.FLOAT32, 0.5).tolist() == [0x3F000000, 0x00000000, 0x7F800000]


@pytest.mark.parametrize("ft", C.FTS)
def test_premises_of_the_gpu_cases(ft):
    """no product of a case word and a case factor is NaN (the words are finite, the factors finite): the GPU tests may
    compare every word bit for bit; and the factors reach every branch of the rounding"""
    seen = {"inf": False, "f32 denormal": False, "f16 denormal": False}
    for case, _ in C.all_cases(ft):
        for w in case.words:
            assert C.finite(ft, w).all(), case.tag
            for f in FACTORS:
                out = S.scaled_ref(w, ft, f)
                assert not S.is_nan(out, ft).any(), f"{case.tag}: a NaN at factor {float(f)!r}"
                if f == FACTORS[3]:
                    seen["inf"] |= bool(S.is_inf(out, ft).any())
                if f == FACTORS[2]:
                    wide = (w.astype(np.uint32) << 16) if ft == S.BFLOAT16 else (w if ft == S.FLOAT32 else None)
                    if wide is not None:
                        with np.errstate(all="ignore"):
                            p = (wide.view(np.float32) * f).view(np.uint32) & 0x7FFFFFFF
                        seen["f32 denormal"] |= bool(((p > 0) & (p < 0x00800000)).any())
                    else:
                        mag = out & 0x7FFF
                        seen["f16 denormal"] |= bool(((mag > 0) & (mag < 0x0400)).any())
    assert seen["inf"], "3.0e38 must produce infinities"
    if ft == S.FLOAT16:
        assert seen["f16 denormal"], "2^-20 must produce float16 denormals"
    else:
        assert seen["f32 denormal"], "2^-20 must produce float32 denormals"


def test_entry_point_is_exported_and_bound():
    import dietgpu_amd

    name = "dgpu_float_decode_scaled"
    raw = ctypes.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    assert name in dietgpu_amd.EXPORTED_SYMBOLS
    assert hasattr(raw, name)
    assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int
    assert callable(dietgpu_amd.decompress_data_scaled)
    from dietgpu_amd import distributed
    import inspect

    assert "scale" in inspect.signature(distributed.GpuFloatCodec.decompress).parameters
    assert "scale" in inspect.signature(distributed.compressed_all_gather).parameters
    assert "clip_norm" in inspect.signature(distributed.compressed_all_reduce).parameters


def test_argument_errors_of_the_c_abi_need_no_device():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    f = L.dgpu_float_decode_scaled
    one = (ctypes.c_uint32 * 1)(16)
    ptr = (ctypes.c_void_p * 1)(0)
    dummy = ctypes.c_void_p(4096)  # a "device" address that is never followed: every call below fails before a launch

    def fails(message, ft, P, n, ins, in_bytes, outs, caps, scale, scale_dev, stride):
        assert f(None, 0, None, ft, P, n, ins, in_bytes, outs, caps, scale, scale_dev, stride, None, None, None) == 1
        assert message in L.dgpu_last_error().decode(), L.dgpu_last_error().decode()

    fails("probBits must be 9, 10 or 11", 2, 12, 1, ptr, one, ptr, one, 0.5, None, 0)
    fails("probBits must be 9, 10 or 11", 2, 8, 1, ptr, one, ptr, one, 0.5, None, 0)
    fails("numInBatch must be <= 65535", 2, 10, 65536, ptr, one, ptr, one, 0.5, None, 0)
    fails("floatType", 0, 10, 1, ptr, one, ptr, one, 0.5, None, 0)
    fails("floatType", 4, 10, 1, ptr, one, ptr, one, 0.5, None, 0)
    fails("scaleStride", 2, 10, 1, ptr, one, ptr, one, 0.5, dummy, 2)
    fails("scaleStride", 2, 10, 1, ptr, one, ptr, one, 0.5, None, 7)
    for bad in (0.0, -0.0, float("inf"), float("-inf"), float("nan")):
        fails("finite and not zero", 2, 10, 1, ptr, one, ptr, one, bad, None, 0)
    fails("scale_dev must be 4-byte aligned", 2, 10, 1, ptr, one, ptr, one, 0.5, ctypes.c_void_p(4098), 0)
    for missing in range(4):
        arrays = [ptr, one, ptr, one]
        arrays[missing] = None
        fails("null array", 2, 10, 1, *arrays, 0.5, None, 0)
        fails("null array", 2, 10, 1, *arrays, 0.0, dummy, 1)  # (a host scale is not looked at beside a device one)
    fails("16-byte aligned", 2, 10, 1, (ctypes.c_void_p * 1)(4096 + 8), one, (ctypes.c_void_p * 1)(8192), one, 0.5, None, 0)
    fails("outCapacity", 2, 10, 1, ptr, one, ptr, (ctypes.c_uint32 * 1)(0xfffff001), 0.5, None, 0)
    used = ctypes.c_size_t(77)  # an empty batch is fine and uses nothing
    assert f(None, 0, ctypes.byref(used), 2, 10, 0, None, None, None, None, 0.5, None, 0, None, None, None) == 0
    assert used.value == 0


@pytest.mark.parametrize("torch_ops", [True, False])
def test_rejects_bad_arguments_without_a_gpu(torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        arch = torch.zeros(1024, dtype=torch.uint8)  # CPU tensors
        out = torch.zeros(4096, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            dg.decompress_data_scaled([arch], [out], 0.5)
        with pytest.raises(RuntimeError):
            dg.decompress_data_scaled([arch], [out], torch.ones(1, dtype=torch.float32))
        with pytest.raises(RuntimeError):
            dg.decompress_data_scaled([arch, arch], [out], 0.5)
        with pytest.raises(RuntimeError):
            dg.decompress_data_scaled([], [], 0.5)
        with pytest.raises(RuntimeError, match="float32"):  # a scale of another dtype
            dg.decompress_data_scaled([arch], [out], torch.ones(1, dtype=torch.float64))
        for wrong in (0, 2, 3):  # a scale of a wrong length
            with pytest.raises(RuntimeError, match="1 element or one per archive"):
                dg.decompress_data_scaled([arch], [out], torch.ones(wrong, dtype=torch.float32))
        for bad in (0.0, float("inf"), float("-inf"), float("nan"), 1e-60):  # (1e-60: its float32 is zero)
            with pytest.raises(RuntimeError, match="finite and not zero"):
                dg.decompress_data_scaled([arch], [out], bad)
        with pytest.raises(RuntimeError):
            dg.decompress_data_scaled([arch], [out], "a third")
    finally:
        dg.prefer_torch_ops(True)
