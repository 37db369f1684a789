"""The norm calls (dgpu_float_reduce_norm_temp_bytes, dgpu_float_decode_reduce_norm, dgpu_float_reduce_compress_norm),
the parts that need no GPU: the entry points are exported and bound, every argument error is raised with its message
before anything touches a device (the pointers are fake addresses that are never dereferenced), the temp-memory query is
monotone, and the `out_sumsq` / `out_nonfinite` keywords of the Python layer check dtype, shape and device."""
import ctypes
import inspect
import math

import pytest
import torch

A = 0x10000  # a fake device address, aligned to everything
THIRD = 1.0 / 3.0


def test_norm_entry_points_are_exported_and_bound():
    import dietgpu_amd
    from dietgpu_amd import _lib, distributed

    raw = ctypes.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    for name in ("dgpu_float_reduce_norm_temp_bytes", "dgpu_float_decode_reduce_norm", "dgpu_float_reduce_compress_norm"):
        assert name in dietgpu_amd.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
    assert L.dgpu_float_reduce_norm_temp_bytes.restype is ctypes.c_size_t
    for name in ("dgpu_float_decode_reduce_norm", "dgpu_float_reduce_compress_norm"):
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int
        # the scaled call's arguments with the two output pointers in front of the stream
        scaled = list(_lib._SIGS[name.replace("_norm", "_scaled")][1])
        assert list(fn.argtypes) == scaled[:-1] + [ctypes.c_void_p, ctypes.c_void_p] + scaled[-1:]
        assert fn.argtypes[11] is ctypes.c_float
    assert L.dgpu_abi_version() == 8  # added entry points do not move the version
    for f in (dietgpu_amd.decompress_data_reduce, dietgpu_amd.decompress_data_reduce_mixed, dietgpu_amd.decompress_data_reduce_compress,
              dietgpu_amd.decompress_data_reduce_compress_mixed):
        p = inspect.signature(f).parameters
        assert p["out_sumsq"].default is None and p["out_nonfinite"].default is None
    for name in ("decompress_reduce", "decompress_reduce_mixed", "decompress_reduce_compress", "decompress_reduce_compress_mixed"):
        assert inspect.signature(getattr(distributed.GpuFloatCodec, name)).parameters["norm"].default is None
    for f in (distributed.compressed_reduce_scatter, distributed.compressed_all_reduce):
        assert inspect.signature(f).parameters["norm"].default is False


def _ptrs(*values):
    return (ctypes.c_void_p * len(values))(*values)


def _u32(*values):
    return (ctypes.c_uint32 * len(values))(*values)


def _u8(*values):
    return (ctypes.c_uint8 * len(values))(*values)


#   floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, sourceKind, scale, out / acc, outCapacity[, outArchive]
def _reduce(L, *args, sumsq=5 * A, nonfinite=6 * A):
    used = ctypes.c_size_t(77)
    return L.dgpu_float_decode_reduce_norm(None, 0, ctypes.byref(used), *args, None, None, sumsq, nonfinite, None)


def _reduce_compress(L, *args, sumsq=5 * A, nonfinite=6 * A):
    used = ctypes.c_size_t(77)
    return L.dgpu_float_reduce_compress_norm(None, 0, ctypes.byref(used), *args, None, None, None, sumsq, nonfinite, None)


def _fails(L, call, message, *args, **kw):
    assert call(L, *args, **kw) == 1  # DGPU_ERR_INVALID_ARGUMENT
    text = L.dgpu_last_error().decode()
    assert text and message in text, text


@pytest.mark.parametrize("scale", [math.nan, math.inf, -math.inf, 0.0, -0.0])
def test_a_scale_that_is_not_finite_or_is_zero_is_an_invalid_argument(scale):
    import dietgpu_amd

    L = dietgpu_amd.lib()
    src, two, kinds, acc, one, arch = _ptrs(A, A), _u32(16, 16), _u8(0, 1), _ptrs(2 * A), _u32(4096), _ptrs(3 * A)
    for k in (kinds, None):
        _fails(L, _reduce, "scale must be finite and not zero", 2, 10, 0, 1, 2, src, two, k, scale, acc, one)
        _fails(L, _reduce_compress, "scale must be finite and not zero", 2, 10, 0, 1, 2, src, two, k, scale, acc, one, arch)
    _fails(L, _reduce, "scale must be finite and not zero", 2, 10, 0, 0, 2, None, None, None, scale, None, None)


@pytest.mark.parametrize("scale", [THIRD, 1.0])
@pytest.mark.parametrize("outputs", [{}, {"nonfinite": None}, {"sumsq": None}, {"sumsq": None, "nonfinite": None}])
def test_every_argument_error_is_raised_before_anything_is_enqueued(scale, outputs):
    """with both outputs, with either, and with neither (the scaled call): what the scaled calls reject is rejected, with
    their messages"""
    import dietgpu_amd

    L = dietgpu_amd.lib()
    src, two, kinds, acc, one, arch = _ptrs(A, A), _u32(16, 16), _u8(0, 1), _ptrs(2 * A), _u32(4096), _ptrs(3 * A)
    for call, tail in ((_reduce, ()), (_reduce_compress, (arch,))):
        def fails(message, *args):
            _fails(L, call, message, *args, *tail, **outputs)

        fails("probBits must be 9, 10 or 11", 2, 12, 1, 1, 2, src, two, kinds, scale, acc, one)
        fails("floatType", 4, 10, 1, 1, 2, src, two, kinds, scale, acc, one)
        fails("accumulate must be 0 or 1", 2, 10, 2, 1, 2, src, two, kinds, scale, acc, one)
        fails("numSources must be between 1 and 64", 2, 10, 1, 1, 0, src, two, kinds, scale, acc, one)
        fails("numSources must be between 1 and 64", 2, 10, 1, 1, 65, src, two, kinds, scale, acc, one)
        fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 32768, 2, src, two, kinds, scale, acc, one)
        fails("null array", 2, 10, 1, 1, 2, None, two, kinds, scale, acc, one)
        fails("null array", 2, 10, 1, 1, 2, src, two, kinds, scale, None, one)
        fails("accumulators must be 4-byte aligned", 2, 10, 1, 1, 2, src, two, kinds, scale, _ptrs(2 * A + 2), one)
        fails("sourceKind must be 0 (archive) or 1 (raw row)", 2, 10, 1, 1, 2, src, two, _u8(0, 2), scale, acc, one)
        fails("raw source must be float-word aligned", 2, 10, 1, 1, 2, _ptrs(A, A + 1), two, kinds, scale, acc, one)
        fails("inBytes of a raw source must be a multiple of the float word size", 2, 10, 1, 1, 2, src, _u32(16, 17), kinds, scale, acc, one)
        fails("compressed input must be 16-byte aligned", 2, 10, 1, 1, 2, _ptrs(A, A + 2), two, None, scale, acc, one)
    _fails(L, _reduce_compress, "floatType must be float16 or bfloat16", 3, 10, 1, 1, 2, src, two, kinds, scale, acc, one, arch, **outputs)
    _fails(L, _reduce_compress, "compressed output must be 16-byte aligned", 2, 10, 1, 1, 2, src, two, kinds, scale, acc, one, _ptrs(3 * A + 8), **outputs)


@pytest.mark.parametrize("scale", [THIRD, 1.0])
def test_misaligned_outputs_are_invalid_arguments(scale):
    import dietgpu_amd

    L = dietgpu_amd.lib()
    src, two, kinds, acc, one, arch = _ptrs(A, A), _u32(16, 16), _u8(0, 1), _ptrs(2 * A), _u32(4096), _ptrs(3 * A)
    for off in (1, 2, 4, 7):
        _fails(L, _reduce, "outSumSq_dev must be 8-byte aligned", 2, 10, 0, 1, 2, src, two, kinds, scale, acc, one, sumsq=5 * A + off)
        _fails(L, _reduce_compress, "outSumSq_dev must be 8-byte aligned", 2, 10, 0, 1, 2, src, two, None, scale, acc, one, arch, sumsq=5 * A + off)
        _fails(L, _reduce, "outSumSq_dev must be 8-byte aligned", 2, 10, 0, 1, 2, src, two, kinds, scale, acc, one, sumsq=5 * A + off, nonfinite=None)
    for off in (1, 2, 3):
        _fails(L, _reduce, "outNonFinite_dev must be 4-byte aligned", 2, 10, 0, 1, 2, src, two, kinds, scale, acc, one, nonfinite=6 * A + off)
        _fails(L, _reduce_compress, "outNonFinite_dev must be 4-byte aligned", 2, 10, 0, 1, 2, src, two, kinds, scale, acc, one, arch, sumsq=None,
               nonfinite=6 * A + off)


@pytest.mark.parametrize("sources", [1, 2, 64])
@pytest.mark.parametrize("ft", [1, 2, 3])
def test_an_empty_batch_is_ok_and_uses_nothing(ft, sources):
    import dietgpu_amd

    L = dietgpu_amd.lib()
    for scale in (THIRD, 1.0):
        used = ctypes.c_size_t(77)
        rc = L.dgpu_float_decode_reduce_norm(None, 0, ctypes.byref(used), ft, 10, 0, 0, sources, None, None, None, scale, None, None, None, None,
                                             5 * A, 6 * A, None)
        assert rc == 0 and used.value == 0, L.dgpu_last_error()
        if ft != 3:
            used = ctypes.c_size_t(77)
            rc = L.dgpu_float_reduce_compress_norm(None, 0, ctypes.byref(used), ft, 10, 0, 0, sources, None, None, None, scale, None, None, None,
                                                   None, None, None, 5 * A, 6 * A, None)
            assert rc == 0 and used.value == 0, L.dgpu_last_error()


def test_the_temp_bytes_query_is_monotone():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    for ft in (1, 2, 3):
        for compress in (0, 1):
            if ft == 3 and compress:
                continue
            q = lambda B, n: L.dgpu_float_reduce_norm_temp_bytes(ft, B, n, compress)
            words = [1, 4096, 4097, 8 * 4096, 8 * 4096 + 1, 16 * 4096 + 1, 512 * 1024, 64 * 1024 * 1024]
            batches = [1, 2, 7, 64, 65, 1000, 65535]
            for B in batches:
                sizes = [q(B, n) for n in words]
                assert sizes == sorted(sizes) and sizes[0] > 0, (ft, compress, B, sizes)
            for n in words:
                sizes = [q(B, n) for B in batches]
                assert sizes == sorted(sizes), (ft, compress, n, sizes)
            # one float64 and one uint32 per member and 16-block tile of the largest member, and the compress side's own
            assert q(32, 512 * 1024) - (L.dgpu_float_reduce_compress_temp_bytes(ft, 32, 512 * 1024) if compress else 0) >= 32 * 8 * 12


@pytest.mark.parametrize("torch_ops", [True, False])
def test_ops_raise_for_outputs_of_the_wrong_dtype_shape_or_device(torch_ops):
    """before anything else is looked at: dtype, then shape, then device (these are CPU tensors: a right one fails for
    that)"""
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        arch = torch.zeros(1024, dtype=torch.uint8)
        acc = torch.zeros(4096, dtype=torch.float32)
        good_sq, good_nf = torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int32)
        for f in (dg.decompress_data_reduce, dg.decompress_data_reduce_mixed, dg.decompress_data_reduce_compress,
                  dg.decompress_data_reduce_compress_mixed):
            def call(**kw):
                f([[arch, arch]], [acc], dtype=torch.bfloat16, **kw)

            for bad in (torch.zeros(1, dtype=torch.float32), torch.zeros(1, dtype=torch.int64), [0.0]):
                with pytest.raises(RuntimeError, match="out_sumsq must be a tensor of dtype float64"):
                    call(out_sumsq=bad, out_nonfinite=good_nf)
            for bad in (torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.float64)):
                with pytest.raises(RuntimeError, match="out_nonfinite must be a tensor of dtype int32"):
                    call(out_sumsq=good_sq, out_nonfinite=bad)
            for bad in (torch.zeros(2, dtype=torch.float64), torch.zeros((1, 1), dtype=torch.float64), torch.zeros(0, dtype=torch.float64)):
                with pytest.raises(RuntimeError, match="out_sumsq must be a contiguous tensor of shape"):
                    call(out_sumsq=bad)
            with pytest.raises(RuntimeError, match="out_nonfinite must be a contiguous tensor of shape"):
                call(out_nonfinite=torch.zeros(3, dtype=torch.int32))
            with pytest.raises(RuntimeError, match="out_sumsq must be on the GPU"):
                call(out_sumsq=good_sq, out_nonfinite=good_nf, scale=THIRD)
            with pytest.raises(RuntimeError, match="out_nonfinite must be on the GPU"):
                call(out_nonfinite=good_nf)
            with pytest.raises(RuntimeError, match="GPU"):  # without the outputs: the checks of today
                call()
    finally:
        dg.prefer_torch_ops(True)
