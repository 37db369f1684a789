"""Decode-accumulate, the parts that need no GPU: the C ABI entry point being exported and bound, its argument checks
(code 1 and a message that names the fault, before anything touches a device) and those of the Python layer."""
import ctypes

import pytest
import torch


def test_accumulate_entry_point_is_exported_and_bound():
    import dietgpu_amd

    name = "dgpu_float_decode_accumulate"
    raw = ctypes.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    assert name in dietgpu_amd.EXPORTED_SYMBOLS
    assert hasattr(raw, name)
    assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int
    assert L.dgpu_abi_version() == 8  # an added entry point does not move the version
    assert callable(dietgpu_amd.decompress_data_accumulate)
    from dietgpu_amd import distributed

    assert callable(distributed.compressed_reduce_scatter)
    assert callable(distributed.GpuFloatCodec.decompress_accumulate)


def test_accumulate_argument_errors_of_the_c_abi_need_no_device():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    f = L.dgpu_float_decode_accumulate
    one = (ctypes.c_uint32 * 1)(16)
    ptr = (ctypes.c_void_p * 1)(0)

    def fails(message, *args):
        assert f(None, 0, None, *args, None, None, None) == 1
        assert message in L.dgpu_last_error().decode()

    #      floatType, probBits, accumulate, numInBatch, in, inBytes, out, outCapacity
    fails("probBits must be 9, 10 or 11", 2, 12, 1, 1, ptr, one, ptr, one)
    fails("probBits must be 9, 10 or 11", 2, 8, 1, 1, ptr, one, ptr, one)
    fails("numInBatch must be <= 65535", 2, 10, 1, 65536, ptr, one, ptr, one)  # (checked before the arrays are read)
    fails("floatType", 0, 10, 1, 1, ptr, one, ptr, one)
    fails("floatType", 4, 10, 1, 1, ptr, one, ptr, one)
    fails("accumulate must be 0 or 1", 2, 10, 2, 1, ptr, one, ptr, one)
    for missing in range(4):
        arrays = [ptr, one, ptr, one]
        arrays[missing] = None
        fails("null array", 2, 10, 1, 1, *arrays)
    fails("16-byte aligned", 2, 10, 1, 1, (ctypes.c_void_p * 1)(4096 + 8), one, (ctypes.c_void_p * 1)(8192), one)
    fails("4-byte aligned", 2, 10, 1, 1, (ctypes.c_void_p * 1)(4096), one, (ctypes.c_void_p * 1)(8192 + 2), one)
    fails("outCapacity", 2, 10, 1, 1, ptr, one, ptr, (ctypes.c_uint32 * 1)(0xfffff001))
    used = ctypes.c_size_t(77)  # an empty batch is fine and uses nothing
    assert f(None, 0, ctypes.byref(used), 2, 10, 1, 0, None, None, None, None, None, None, None) == 0
    assert used.value == 0


@pytest.mark.parametrize("torch_ops", [True, False])
def test_accumulate_rejects_bad_tensors_without_a_gpu(torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        arch = torch.zeros(1024, dtype=torch.uint8)  # CPU tensors
        acc = torch.zeros(4096, dtype=torch.float32)
        with pytest.raises(RuntimeError):
            dg.decompress_data_accumulate([arch], [acc])
        with pytest.raises(RuntimeError):
            dg.decompress_data_accumulate([arch], [acc], accumulate=False, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            dg.decompress_data_accumulate([arch, arch], [acc])
        with pytest.raises(RuntimeError):
            dg.decompress_data_accumulate([], [])
        # accumulators that are not float32
        for bad in (torch.bfloat16, torch.float16, torch.float64, torch.int32):
            with pytest.raises(RuntimeError):
                dg.decompress_data_accumulate([arch], [acc.to(bad)])
    finally:
        dg.prefer_torch_ops(True)
