"""The scaled calls (dgpu_float_decode_reduce_scaled, dgpu_float_reduce_compress_scaled), the parts that need no GPU: the
entry points are exported and bound with a C float for the scale, a scale that is not finite or is zero returns
DGPU_ERR_INVALID_ARGUMENT with a message before anything touches a device (the pointers are fake addresses that are
never dereferenced), the argument errors of the mixed calls still fire with a scale given, sourceKind may be NULL, the
empty batch, and the `scale` keyword of the Python layer."""
import ctypes
import inspect
import math

import pytest
import torch

A = 0x10000  # a fake device address, aligned to everything
BAD_SCALES = (math.nan, math.inf, -math.inf, 0.0, -0.0)
THIRD = 1.0 / 3.0


def test_scaled_entry_points_are_exported_and_bound():
    import dietgpu_amd
    from dietgpu_amd import _lib, distributed

    raw = ctypes.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    for name in ("dgpu_float_decode_reduce_scaled", "dgpu_float_reduce_compress_scaled"):
        assert name in dietgpu_amd.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int
        # the scale sits behind sourceKind, as a C float: without an explicit c_float ctypes would pass a double
        assert fn.argtypes[11] is ctypes.c_float and fn.argtypes.count(ctypes.c_float) == 1
        mixed = _lib._SIGS[name.replace("_scaled", "_mixed")][1]
        assert list(fn.argtypes[:11]) + list(fn.argtypes[12:]) == list(mixed)
    assert L.dgpu_abi_version() == 8  # added entry points do not move the version
    for f in (dietgpu_amd.decompress_data_reduce, dietgpu_amd.decompress_data_reduce_mixed, dietgpu_amd.decompress_data_reduce_compress,
              dietgpu_amd.decompress_data_reduce_compress_mixed):
        assert inspect.signature(f).parameters["scale"].default is None
    for name in ("decompress_reduce", "decompress_reduce_mixed", "decompress_reduce_compress", "decompress_reduce_compress_mixed"):
        assert inspect.signature(getattr(distributed.GpuFloatCodec, name)).parameters["scale"].default is None
    for f in (distributed.compressed_reduce_scatter, distributed.compressed_all_reduce):
        p = inspect.signature(f).parameters
        assert p["op"].default == "sum" and p["scale"].default is None


def _ptrs(*values):
    return (ctypes.c_void_p * len(values))(*values)


def _u32(*values):
    return (ctypes.c_uint32 * len(values))(*values)


def _u8(*values):
    return (ctypes.c_uint8 * len(values))(*values)


#   floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, sourceKind, scale, out / acc, outCapacity[, outArchive]
def _reduce(L, *args):
    used = ctypes.c_size_t(77)
    return L.dgpu_float_decode_reduce_scaled(None, 0, ctypes.byref(used), *args, None, None, None)


def _reduce_compress(L, *args):
    used = ctypes.c_size_t(77)
    return L.dgpu_float_reduce_compress_scaled(None, 0, ctypes.byref(used), *args, None, None, None, None)


def _fails(L, call, message, *args):
    assert call(L, *args) == 1  # DGPU_ERR_INVALID_ARGUMENT
    text = L.dgpu_last_error().decode()
    assert text and message in text, text


@pytest.mark.parametrize("scale", BAD_SCALES)
def test_a_scale_that_is_not_finite_or_is_zero_is_an_invalid_argument(scale):
    import dietgpu_amd

    L = dietgpu_amd.lib()
    src, two, kinds, acc, one, arch = _ptrs(A, A), _u32(16, 16), _u8(0, 1), _ptrs(2 * A), _u32(4096), _ptrs(3 * A)
    for k in (kinds, None):
        _fails(L, _reduce, "scale must be finite and not zero", 2, 10, 0, 1, 2, src, two, k, scale, acc, one)
        _fails(L, _reduce_compress, "scale must be finite and not zero", 2, 10, 0, 1, 2, src, two, k, scale, acc, one, arch)
    # ... for an empty batch too: the scale is a scalar of the call like probBits
    _fails(L, _reduce, "scale must be finite and not zero", 2, 10, 0, 0, 2, None, None, None, scale, None, None)
    _fails(L, _reduce_compress, "scale must be finite and not zero", 2, 10, 0, 0, 2, None, None, None, scale, None, None, None)


@pytest.mark.parametrize("scale", [THIRD, 1.0])
def test_the_argument_errors_of_the_mixed_calls_still_fire(scale):
    """with a scale (and with 1.0, which forwards): what the unscaled calls reject is rejected, with their messages"""
    import dietgpu_amd

    L = dietgpu_amd.lib()
    src, two, kinds, acc, one, arch = _ptrs(A, A), _u32(16, 16), _u8(0, 1), _ptrs(2 * A), _u32(4096), _ptrs(3 * A)
    for call, tail in ((_reduce, ()), (_reduce_compress, (arch,))):
        def fails(message, *args):
            _fails(L, call, message, *args, *tail)

        fails("probBits must be 9, 10 or 11", 2, 12, 1, 1, 2, src, two, kinds, scale, acc, one)
        fails("floatType", 4, 10, 1, 1, 2, src, two, kinds, scale, acc, one)
        fails("accumulate must be 0 or 1", 2, 10, 2, 1, 2, src, two, kinds, scale, acc, one)
        fails("numSources must be between 1 and 64", 2, 10, 1, 1, 0, src, two, kinds, scale, acc, one)
        fails("numSources must be between 1 and 64", 2, 10, 1, 1, 65, src, two, kinds, scale, acc, one)
        fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 32768, 2, src, two, kinds, scale, acc, one)
        fails("null array", 2, 10, 1, 1, 2, None, two, kinds, scale, acc, one)
        fails("accumulators must be 4-byte aligned", 2, 10, 1, 1, 2, src, two, kinds, scale, _ptrs(2 * A + 2), one)
        fails("sourceKind must be 0 (archive) or 1 (raw row)", 2, 10, 1, 1, 2, src, two, _u8(0, 2), scale, acc, one)
        fails("sourceKind must be 0 (archive) or 1 (raw row)", 2, 10, 1, 1, 2, src, two, _u8(255, 0), scale, acc, one)
        fails("raw source must be float-word aligned", 2, 10, 1, 1, 2, _ptrs(A, A + 1), two, kinds, scale, acc, one)
        fails("raw source must be float-word aligned", 2, 10, 0, 1, 1, _ptrs(A + 1), _u32(16), _u8(1), scale, acc, one)  # one source too
        fails("inBytes of a raw source must be a multiple of the float word size", 2, 10, 1, 1, 2, src, _u32(16, 17), kinds, scale, acc, one)
        # 16-byte alignment: of archive sources only, and of every source when sourceKind is NULL
        fails("compressed input must be 16-byte aligned", 2, 10, 1, 1, 2, _ptrs(A + 8, A), two, kinds, scale, acc, one)
        fails("compressed input must be 16-byte aligned", 2, 10, 1, 1, 2, _ptrs(A, A + 2), two, None, scale, acc, one)
    _fails(L, _reduce_compress, "floatType must be float16 or bfloat16", 3, 10, 1, 1, 2, src, two, kinds, scale, acc, one, arch)
    _fails(L, _reduce_compress, "compressed output must be 16-byte aligned", 2, 10, 1, 1, 2, src, two, kinds, scale, acc, one, _ptrs(3 * A + 8))


@pytest.mark.parametrize("scale", [THIRD, 0.5, -3.0, 2.0 ** -20, 1.0])
@pytest.mark.parametrize("sources", [1, 2, 64])
@pytest.mark.parametrize("ft", [1, 2, 3])
def test_an_empty_batch_is_ok_and_uses_nothing(ft, sources, scale):
    """... with sourceKind NULL, which is accepted: every source is an archive"""
    import dietgpu_amd

    L = dietgpu_amd.lib()
    used = ctypes.c_size_t(77)
    rc = L.dgpu_float_decode_reduce_scaled(None, 0, ctypes.byref(used), ft, 10, 0, 0, sources, None, None, None, scale, None, None, None, None, None)
    assert rc == 0 and used.value == 0, L.dgpu_last_error()
    if ft != 3:
        used = ctypes.c_size_t(77)
        rc = L.dgpu_float_reduce_compress_scaled(None, 0, ctypes.byref(used), ft, 10, 0, 0, sources, None, None, None, scale, None, None, None,
                                                 None, None, None, None)
        assert rc == 0 and used.value == 0, L.dgpu_last_error()


@pytest.mark.parametrize("torch_ops", [True, False])
@pytest.mark.parametrize("scale", BAD_SCALES + (1e-60, 1e60))
def test_ops_raise_for_a_scale_that_is_not_finite_or_is_zero(scale, torch_ops):
    """on both routes, and before anything else is looked at; 1e-60 and 1e60 are zero and infinite as float32"""
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        arch = torch.zeros(1024, dtype=torch.uint8)
        acc = torch.zeros(4096, dtype=torch.float32)
        for f in (dg.decompress_data_reduce, dg.decompress_data_reduce_mixed, dg.decompress_data_reduce_compress,
                  dg.decompress_data_reduce_compress_mixed):
            with pytest.raises(RuntimeError, match="scale must be finite and not zero"):
                f([[arch, arch]], [acc], dtype=torch.bfloat16, scale=scale)
    finally:
        dg.prefer_torch_ops(True)


def test_a_good_scale_leaves_the_other_checks_of_ops_in_place():
    import dietgpu_amd as dg

    arch = torch.zeros(1024, dtype=torch.uint8)  # CPU tensors
    acc = torch.zeros(4096, dtype=torch.float32)
    for f in (dg.decompress_data_reduce, dg.decompress_data_reduce_mixed, dg.decompress_data_reduce_compress,
              dg.decompress_data_reduce_compress_mixed):
        for scale in (THIRD, 1.0, None):
            with pytest.raises(RuntimeError, match="GPU"):
                f([[arch, arch]], [acc], dtype=torch.bfloat16, scale=scale)
            with pytest.raises(RuntimeError):
                f([[arch] * 65], [acc], dtype=torch.bfloat16, scale=scale)


def test_the_scale_of_ops_is_rounded_once_to_float32():
    from dietgpu_amd import ops

    assert ops._scale32(None) is None and ops._scale32(1.0) is None and ops._scale32(1.0 + 2.0 ** -30) is None
    f = ops._scale32(THIRD)
    assert f == ctypes.c_float(THIRD).value and f != THIRD
    assert ops._scale32(-3) == -3.0
