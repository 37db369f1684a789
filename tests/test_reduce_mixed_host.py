"""The mixed-source calls (dgpu_float_decode_reduce_mixed, dgpu_float_reduce_compress_mixed), the parts that need no
GPU: the entry points are exported and bound, every invalid argument of the contract returns DGPU_ERR_INVALID_ARGUMENT
with a message before anything touches a device (the library loads without one, the pointers are fake addresses that
are never dereferenced), the empty batch, and the argument checks of the Python layer on CPU tensors."""
import ctypes

import pytest
import torch

A = 0x10000  # a fake device address, aligned to everything


def test_mixed_entry_points_are_exported_and_bound():
    import dietgpu_amd
    from dietgpu_amd import distributed

    raw = ctypes.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    for name in ("dgpu_float_decode_reduce_mixed", "dgpu_float_reduce_compress_mixed"):
        assert name in dietgpu_amd.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int
    assert L.dgpu_abi_version() == 8  # added entry points do not move the version
    assert callable(dietgpu_amd.decompress_data_reduce_mixed) and callable(dietgpu_amd.decompress_data_reduce_compress_mixed)
    assert callable(distributed.GpuFloatCodec.decompress_reduce_mixed)
    assert callable(distributed.GpuFloatCodec.decompress_reduce_compress_mixed)


def _ptrs(*values):
    return (ctypes.c_void_p * len(values))(*values)


def _u32(*values):
    return (ctypes.c_uint32 * len(values))(*values)


def _u8(*values):
    return (ctypes.c_uint8 * len(values))(*values)


def _reduce(L, *args):
    used = ctypes.c_size_t(77)
    return L.dgpu_float_decode_reduce_mixed(None, 0, ctypes.byref(used), *args, None, None, None)


def _reduce_compress(L, *args):
    used = ctypes.c_size_t(77)
    return L.dgpu_float_reduce_compress_mixed(None, 0, ctypes.byref(used), *args, None, None, None, None)


def test_decode_reduce_mixed_argument_errors_need_no_device():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    src, two, kinds, acc, one = _ptrs(A, A), _u32(16, 16), _u8(0, 1), _ptrs(2 * A), _u32(4096)

    def fails(message, *args):
        assert _reduce(L, *args) == 1  # DGPU_ERR_INVALID_ARGUMENT
        text = L.dgpu_last_error().decode()
        assert text and message in text, text

    #      floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, sourceKind, out, outCapacity
    # the checks of dgpu_float_decode_reduce apply
    fails("probBits must be 9, 10 or 11", 2, 12, 1, 1, 2, src, two, kinds, acc, one)
    fails("floatType", 0, 10, 1, 1, 2, src, two, kinds, acc, one)
    fails("floatType", 4, 10, 1, 1, 2, src, two, kinds, acc, one)
    fails("accumulate must be 0 or 1", 2, 10, 2, 1, 2, src, two, kinds, acc, one)
    fails("numSources must be between 1 and 64", 2, 10, 1, 1, 0, src, two, kinds, acc, one)
    fails("numSources must be between 1 and 64", 2, 10, 1, 1, 65, src, two, kinds, acc, one)
    fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 32768, 2, src, two, kinds, acc, one)
    for missing in (0, 1, 3, 4):
        arrays = [src, two, kinds, acc, one]
        arrays[missing] = None
        fails("null array", 2, 10, 1, 1, 2, *arrays)
    fails("accumulators must be 4-byte aligned", 2, 10, 1, 1, 2, src, two, kinds, _ptrs(2 * A + 2), one)
    fails("outCapacity must not exceed 0xfffff000", 2, 10, 1, 1, 2, src, two, kinds, acc, _u32(0xFFFFF001))
    # ... and the mixed ones
    fails("sourceKind is null", 2, 10, 1, 1, 2, src, two, None, acc, one)
    fails("sourceKind is null", 2, 10, 1, 1, 1, _ptrs(A), _u32(16), None, acc, one)
    fails("sourceKind must be 0 (archive) or 1 (raw row)", 2, 10, 1, 1, 2, src, two, _u8(0, 2), acc, one)
    fails("sourceKind must be 0 (archive) or 1 (raw row)", 2, 10, 1, 1, 2, src, two, _u8(255, 0), acc, one)
    # 16-byte alignment: of archive sources only
    fails("compressed input must be 16-byte aligned", 2, 10, 1, 1, 2, _ptrs(A + 8, A), two, kinds, acc, one)
    fails("compressed input must be 16-byte aligned", 2, 10, 1, 1, 2, _ptrs(A, A + 2), two, _u8(1, 0), acc, one)
    # a raw row: aligned to the word size, a whole number of words
    fails("raw source must be float-word aligned", 2, 10, 1, 1, 2, _ptrs(A, A + 1), two, kinds, acc, one)
    fails("raw source must be float-word aligned", 1, 10, 1, 1, 2, _ptrs(A, A + 3), two, kinds, acc, one)
    fails("raw source must be float-word aligned", 3, 10, 1, 1, 2, _ptrs(A, A + 2), two, kinds, acc, one)  # float32: 4 bytes
    fails("raw source must be float-word aligned", 2, 10, 0, 1, 1, _ptrs(A + 1), _u32(16), _u8(1), acc, one)  # one source: this call too
    fails("inBytes of a raw source must be a multiple of the float word size", 2, 10, 1, 1, 2, src, _u32(16, 17), kinds, acc, one)
    fails("inBytes of a raw source must be a multiple of the float word size", 3, 10, 1, 1, 2, src, _u32(16, 18), kinds, acc, one)
    fails("inBytes of a raw source must be a multiple of the float word size", 3, 10, 1, 1, 2, src, _u32(18, 16), _u8(1, 1), acc, one)


def test_reduce_compress_mixed_argument_errors_need_no_device():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    src, two, kinds, acc, one, arch = _ptrs(A, A), _u32(16, 16), _u8(1, 0), _ptrs(2 * A), _u32(4096), _ptrs(3 * A)

    def fails(message, *args):
        assert _reduce_compress(L, *args) == 1
        text = L.dgpu_last_error().decode()
        assert text and message in text, text

    #      floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, sourceKind, acc, outCapacity, outArchive
    fails("probBits must be 9, 10 or 11", 2, 8, 1, 1, 2, src, two, kinds, acc, one, arch)
    fails("floatType must be float16 or bfloat16", 3, 10, 1, 1, 2, src, two, kinds, acc, one, arch)
    fails("accumulate must be 0 or 1", 2, 10, -1, 1, 2, src, two, kinds, acc, one, arch)
    fails("numSources must be between 1 and 64", 2, 10, 1, 1, 65, src, two, kinds, acc, one, arch)
    fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 1024, 64, src, two, kinds, acc, one, arch)
    for missing in (0, 1, 3, 4, 5):
        arrays = [src, two, kinds, acc, one, arch]
        arrays[missing] = None
        fails("null array", 2, 10, 1, 1, 2, *arrays)
    fails("accumulators must be 4-byte aligned", 2, 10, 1, 1, 2, src, two, kinds, _ptrs(2 * A + 2), one, arch)
    fails("compressed output must be 16-byte aligned", 2, 10, 1, 1, 2, src, two, kinds, acc, one, _ptrs(3 * A + 8))
    fails("outCapacity larger than 1717538816 words", 2, 10, 1, 1, 2, src, two, kinds, acc, _u32(1717538816 + 1), arch)
    fails("sourceKind is null", 2, 10, 1, 1, 2, src, two, None, acc, one, arch)
    fails("sourceKind must be 0 (archive) or 1 (raw row)", 1, 10, 1, 1, 2, src, two, _u8(1, 3), acc, one, arch)
    fails("compressed input must be 16-byte aligned", 2, 10, 1, 1, 2, _ptrs(A + 2, A + 2), two, kinds, acc, one, arch)  # the archive of the two
    fails("raw source must be float-word aligned", 2, 10, 1, 1, 2, _ptrs(A + 1, A), two, kinds, acc, one, arch)
    fails("inBytes of a raw source must be a multiple of the float word size", 1, 10, 1, 1, 2, src, _u32(15, 16), kinds, acc, one, arch)


@pytest.mark.parametrize("sources", [1, 2, 64])
@pytest.mark.parametrize("ft", [1, 2, 3])
def test_an_empty_batch_is_ok_and_uses_nothing(ft, sources):
    import dietgpu_amd

    L = dietgpu_amd.lib()
    used = ctypes.c_size_t(77)
    rc = L.dgpu_float_decode_reduce_mixed(None, 0, ctypes.byref(used), ft, 10, 0, 0, sources, None, None, None, None, None, None, None, None)
    assert rc == 0 and used.value == 0
    if ft != 3:
        used = ctypes.c_size_t(77)
        rc = L.dgpu_float_reduce_compress_mixed(None, 0, ctypes.byref(used), ft, 10, 0, 0, sources, None, None, None, None, None, None, None,
                                                None, None, None)
        assert rc == 0 and used.value == 0


def test_an_empty_batch_still_has_its_scalars_checked():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    for args, message in (((4, 10, 0, 0, 2), "floatType"), ((2, 7, 0, 0, 2), "probBits"), ((2, 10, 3, 0, 2), "accumulate"),
                          ((2, 10, 0, 0, 65), "numSources")):
        assert L.dgpu_float_decode_reduce_mixed(None, 0, None, *args, None, None, None, None, None, None, None, None) == 1
        assert message in L.dgpu_last_error().decode()
        assert L.dgpu_float_reduce_compress_mixed(None, 0, None, *args, None, None, None, None, None, None, None, None, None, None) == 1
        assert message in L.dgpu_last_error().decode()


@pytest.mark.parametrize("torch_ops", [True, False])
def test_mixed_ops_reject_bad_tensors_without_a_gpu(torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        arch = torch.zeros(1024, dtype=torch.uint8)  # CPU tensors
        row = torch.zeros(4096, dtype=torch.bfloat16)
        acc = torch.zeros(4096, dtype=torch.float32)
        for f in (dg.decompress_data_reduce_mixed, dg.decompress_data_reduce_compress_mixed):
            with pytest.raises(RuntimeError):  # not on the GPU
                f([[arch, row]], [acc], dtype=torch.bfloat16)
            with pytest.raises(RuntimeError):  # ragged source lists
                f([[arch, row], [row]], [acc, acc.clone()], dtype=torch.bfloat16)
            with pytest.raises(RuntimeError):  # empty lists
                f([], [])
            with pytest.raises(RuntimeError):
                f([[]], [acc], dtype=torch.bfloat16)
            with pytest.raises(RuntimeError):  # one list of sources per accumulator
                f([[arch, row], [arch, row]], [acc], dtype=torch.bfloat16)
            with pytest.raises(RuntimeError):
                f([[row] * 65], [acc], dtype=torch.bfloat16)
            with pytest.raises(RuntimeError):
                f([[arch, row]], [acc], dtype=torch.float64)
        with pytest.raises(RuntimeError):  # float32 sources: there is no cast to do
            dg.decompress_data_reduce_compress_mixed([[arch, row.to(torch.float32)]], [acc], dtype=torch.float32)
    finally:
        dg.prefer_torch_ops(True)


def test_a_raw_source_of_another_dtype_is_a_runtime_error():
    """checked before the device is: a source is a uint8 archive or a row of the call's float dtype, 1-D"""
    import dietgpu_amd.ops as ops

    arch = torch.zeros(64, dtype=torch.uint8)
    acc = torch.zeros(32, dtype=torch.float32)
    with pytest.raises(RuntimeError):
        ops.decompress_data_reduce_mixed([[arch, torch.zeros(32, dtype=torch.float16)]], [acc], dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.decompress_data_reduce_mixed([[arch, torch.zeros(32, dtype=torch.int16)]], [acc], dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.decompress_data_reduce_mixed([[arch, torch.zeros((2, 16), dtype=torch.bfloat16)]], [acc], dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):  # two raw rows of different dtypes, none given
        ops.decompress_data_reduce_mixed([[torch.zeros(32, dtype=torch.float16), torch.zeros(32, dtype=torch.bfloat16)]], [acc])
