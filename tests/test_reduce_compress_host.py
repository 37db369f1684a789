"""Reduce-compress (dgpu_float_reduce_compress), the parts that need no GPU: the entry points are exported and bound,
every invalid argument of the contract returns DGPU_ERR_INVALID_ARGUMENT with a message before anything touches a
device (the library loads without one, the pointers are fake addresses that are never dereferenced), the empty batch,
the temp-memory query, and the argument checks of the Python layer on CPU tensors."""
import ctypes

import pytest
import torch

A = 0x10000  # a fake device address, aligned to everything
TOO_LARGE = 1717538816 + 1


def test_reduce_compress_entry_points_are_exported_and_bound():
    import dietgpu_amd
    from dietgpu_amd import distributed

    raw = ctypes.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    for name, res in (("dgpu_float_reduce_compress", ctypes.c_int), ("dgpu_float_reduce_compress_temp_bytes", ctypes.c_size_t)):
        assert name in dietgpu_amd.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is res
    assert L.dgpu_abi_version() == 8  # added entry points do not move the version
    assert callable(dietgpu_amd.decompress_data_reduce_compress)
    assert callable(distributed.GpuFloatCodec.decompress_reduce_compress)


def _arrays():
    src = (ctypes.c_void_p * 2)(A, A)  # (sources may alias each other)
    two = (ctypes.c_uint32 * 2)(16, 16)
    acc = (ctypes.c_void_p * 1)(2 * A)
    one = (ctypes.c_uint32 * 1)(4096)
    arch = (ctypes.c_void_p * 1)(3 * A)
    return src, two, acc, one, arch


def test_reduce_compress_argument_errors_need_no_device():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    f = L.dgpu_float_reduce_compress
    src, two, acc, one, arch = _arrays()

    def fails(message, *args):
        used = ctypes.c_size_t(77)
        assert f(None, 0, ctypes.byref(used), *args, None, None, None, None) == 1  # DGPU_ERR_INVALID_ARGUMENT
        text = L.dgpu_last_error().decode()
        assert text and message in text, text

    #      floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, acc, outCapacity, outArchive
    fails("probBits must be 9, 10 or 11", 2, 12, 1, 1, 2, src, two, acc, one, arch)
    fails("probBits must be 9, 10 or 11", 2, 8, 1, 1, 2, src, two, acc, one, arch)
    fails("floatType", 0, 10, 1, 1, 2, src, two, acc, one, arch)
    fails("floatType", 4, 10, 1, 1, 2, src, two, acc, one, arch)
    fails("floatType must be float16 or bfloat16", 3, 10, 1, 1, 2, src, two, acc, one, arch)  # float32: no cast to do
    fails("accumulate must be 0 or 1", 2, 10, 2, 1, 2, src, two, acc, one, arch)
    fails("accumulate must be 0 or 1", 2, 10, -1, 1, 2, src, two, acc, one, arch)
    fails("numSources must be between 1 and 64", 2, 10, 1, 1, 0, src, two, acc, one, arch)
    fails("numSources must be between 1 and 64", 2, 10, 1, 1, 65, src, two, acc, one, arch)
    # (the products are checked before the arrays are read)
    fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 32768, 2, src, two, acc, one, arch)
    fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 1024, 64, src, two, acc, one, arch)
    fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 0xFFFFFFFF, 64, src, two, acc, one, arch)
    fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 65536, 1, src, two, acc, one, arch)
    for missing in range(5):
        arrays = [src, two, acc, one, arch]
        arrays[missing] = None
        fails("null array", 2, 10, 1, 1, 2, *arrays)
    fails("compressed input must be 16-byte aligned", 2, 10, 1, 1, 2, (ctypes.c_void_p * 2)(A, A + 8), two, acc, one, arch)  # the SECOND source
    fails("compressed input must be 16-byte aligned", 2, 10, 1, 1, 2, (ctypes.c_void_p * 2)(A + 4, A), two, acc, one, arch)
    fails("accumulators must be 4-byte aligned", 2, 10, 1, 1, 2, src, two, (ctypes.c_void_p * 1)(2 * A + 2), one, arch)
    fails("compressed output must be 16-byte aligned", 2, 10, 1, 1, 2, src, two, acc, one, (ctypes.c_void_p * 1)(3 * A + 8))
    fails("outCapacity larger than 1717538816 words", 2, 10, 1, 1, 2, src, two, acc, (ctypes.c_uint32 * 1)(TOO_LARGE), arch)
    # numSources == 1 is this call too, with the same checks (it does not forward to decode-accumulate)
    fails("reduce-compress: null array", 2, 10, 1, 1, 1, None, one, acc, one, arch)
    fails("reduce-compress: accumulators must be 4-byte aligned", 1, 10, 0, 1, 1, (ctypes.c_void_p * 1)(A), one,
          (ctypes.c_void_p * 1)(2 * A + 2), one, arch)


@pytest.mark.parametrize("sources", [1, 2, 64])
@pytest.mark.parametrize("ft", [1, 2])
def test_an_empty_batch_is_ok_and_uses_nothing(ft, sources):
    import dietgpu_amd

    used = ctypes.c_size_t(77)
    rc = dietgpu_amd.lib().dgpu_float_reduce_compress(None, 0, ctypes.byref(used), ft, 10, 0, 0, sources, None, None, None, None, None,
                                                      None, None, None, None)
    assert rc == 0 and used.value == 0


def test_an_empty_batch_still_has_its_scalars_checked():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    for args, message in (((3, 10, 0, 0, 2), "floatType"), ((2, 7, 0, 0, 2), "probBits"), ((2, 10, 3, 0, 2), "accumulate"),
                          ((2, 10, 0, 0, 65), "numSources")):
        assert L.dgpu_float_reduce_compress(None, 0, None, *args, None, None, None, None, None, None, None, None, None) == 1
        assert message in L.dgpu_last_error().decode()


def test_temp_bytes_is_monotone_and_covers_the_compress_side():
    import dietgpu_amd

    L = dietgpu_amd.lib()

    def q(ft, B, n):
        return L.dgpu_float_reduce_compress_temp_bytes(ft, B, n)

    batches = (1, 2, 13, 63, 64, 65, 67, 256, 4096)
    words = (1, 4096, 4097, 8 * 4096, 8 * 4096 + 1, 1 << 19, 1 << 24)
    for ft in (1, 2):
        for B in batches:
            for n in words:
                assert q(ft, B, n) >= L.dgpu_float_compress_temp_bytes(ft, B, n), (ft, B, n)
        for n in words:
            sizes = [q(ft, B, n) for B in batches]
            assert sizes == sorted(sizes), (ft, n, sizes)
        for B in batches:
            sizes = [q(ft, B, n) for n in words]
            assert sizes == sorted(sizes), (ft, B, sizes)
        # beyond the 64 members whose counts live in the stream's counters: room for [B][256] counts
        assert q(ft, 65, 4096) - L.dgpu_float_compress_temp_bytes(ft, 65, 4096) >= 65 * 256 * 4
        assert q(ft, 64, 4096) == L.dgpu_float_compress_temp_bytes(ft, 64, 4096)


@pytest.mark.parametrize("torch_ops", [True, False])
def test_reduce_compress_rejects_bad_tensors_without_a_gpu(torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        arch = torch.zeros(1024, dtype=torch.uint8)  # CPU tensors
        acc = torch.zeros(4096, dtype=torch.float32)
        f = dg.decompress_data_reduce_compress
        with pytest.raises(RuntimeError):
            f([[arch, arch]], [acc])
        with pytest.raises(RuntimeError):
            f([[arch, arch]], [acc], accumulate=True, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):  # ragged source lists
            f([[arch, arch], [arch]], [acc, acc.clone()], dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):  # empty lists
            f([], [])
        with pytest.raises(RuntimeError):
            f([[]], [acc], dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):  # one list of sources per accumulator
            f([[arch, arch], [arch, arch]], [acc], dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            f([[arch] * 65], [acc], dtype=torch.bfloat16)
        for bad in (torch.bfloat16, torch.float16, torch.float64, torch.int32):  # accumulators that are not float32
            with pytest.raises(RuntimeError):
                f([[arch, arch]], [acc.to(bad)], dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):  # float32 archives: there is no cast to do
            f([[arch, arch]], [acc], dtype=torch.float32)
    finally:
        dg.prefer_torch_ops(True)
