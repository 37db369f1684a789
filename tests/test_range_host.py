"""Ranged decode, the parts that need no GPU: the block cover of a word range, the two C ABI entry points being
exported and bound, and the argument checks of the Python layer (RuntimeError before anything touches a device)."""
import ctypes

import pytest
import torch


def test_block_cover_at_block_edges():
    from dietgpu_amd import block_cover

    assert block_cover(0, 1) == (0, 1, 0)                  # a single word at the start
    assert block_cover(0, 4096) == (0, 1, 0)               # exactly the first block
    assert block_cover(0, 4097) == (0, 2, 0)
    assert block_cover(4096, 4096) == (1, 1, 0)            # start and end on multiples of 4096
    assert block_cover(8192, 3 * 4096) == (2, 3, 0)
    assert block_cover(4095, 1) == (0, 1, 4095)            # the last word of a block
    assert block_cover(4096, 1) == (1, 1, 0)               # the first word of the next
    assert block_cover(4095, 2) == (0, 2, 4095)            # crosses exactly one boundary
    assert block_cover(5000, 4000) == (1, 2, 904)          # 5000 .. 8999: blocks 1 and 2
    assert block_cover(5000, 3192) == (1, 1, 904)          # ends exactly at 8192
    assert block_cover(0, 0) == (0, 0, 0)                  # a count of 0 covers no block
    assert block_cover(10000, 0) == (2, 0, 1808)
    # never more than 2 x 4095 words beyond the request
    for start, count in [(1, 4096), (4095, 4098), (123, 1), (4097, 8190)]:
        first, blocks, offset = block_cover(start, count)
        assert first * 4096 + offset == start and blocks * 4096 >= offset + count
        assert blocks * 4096 - count <= 2 * 4095
    with pytest.raises(RuntimeError):
        block_cover(-1, 4)
    with pytest.raises(RuntimeError):
        block_cover(0, -4)


def test_range_entry_points_are_exported_and_bound():
    import dietgpu_amd

    names = ("dgpu_ans_decode_batch_pointer_range", "dgpu_float_decompress_range")
    raw = ctypes.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    for n in names:
        assert n in dietgpu_amd.EXPORTED_SYMBOLS
        assert hasattr(raw, n)
        assert getattr(L, n).argtypes is not None and getattr(L, n).restype is ctypes.c_int
    assert L.dgpu_abi_version() == 8
    assert callable(dietgpu_amd.decompress_data_range) and callable(dietgpu_amd.decompress_data_slice)
    from dietgpu_amd import distributed

    assert callable(distributed.decompress_shard)


def test_range_argument_errors_of_the_c_abi_need_no_device():
    # rejected before anything is enqueued: bad probBits, bad float type, too large a batch, null arrays
    import dietgpu_amd

    L = dietgpu_amd.lib()
    one = (ctypes.c_uint32 * 1)(0)
    ptr = (ctypes.c_void_p * 1)(0)
    assert L.dgpu_ans_decode_batch_pointer_range(None, 0, None, 12, 1, ptr, one, one, one, ptr, one, None, None, None) == 1
    assert L.dgpu_float_decompress_range(None, 0, None, 0, 10, 1, ptr, one, one, one, ptr, one, None, None, None) == 1
    assert L.dgpu_float_decompress_range(None, 0, None, 4, 10, 1, ptr, one, one, one, ptr, one, None, None, None) == 1
    assert L.dgpu_ans_decode_batch_pointer_range(None, 0, None, 10, 65536, ptr, one, one, one, ptr, one, None, None, None) == 1
    assert L.dgpu_ans_decode_batch_pointer_range(None, 0, None, 10, 1, None, one, one, one, ptr, one, None, None, None) == 1
    assert L.dgpu_float_decompress_range(None, 0, None, 2, 10, 1, ptr, one, None, one, ptr, one, None, None, None) == 1
    big = (ctypes.c_uint32 * 1)(0xfffff001)  # a capacity whose blocks would round up to 2^32 symbols
    assert L.dgpu_ans_decode_batch_pointer_range(None, 0, None, 10, 1, ptr, one, one, one, ptr, big, None, None, None) == 1
    used = ctypes.c_size_t(77)  # an empty batch is fine and uses nothing
    assert L.dgpu_ans_decode_batch_pointer_range(None, 0, ctypes.byref(used), 10, 0, None, None, None, None, None, None, None, None, None) == 0
    assert used.value == 0


@pytest.mark.parametrize("torch_ops", [True, False])
def test_range_and_slice_reject_bad_arguments_without_a_gpu(torch_ops):
    import dietgpu_amd as dg
    from dietgpu_amd import distributed

    dg.prefer_torch_ops(torch_ops)
    try:
        arch = torch.zeros(1024, dtype=torch.uint8)          # CPU tensors
        out = torch.zeros(4096, dtype=torch.uint8)
        with pytest.raises(RuntimeError):
            dg.decompress_data_range(False, [arch], [out], [0], [1])
        with pytest.raises(RuntimeError):
            dg.decompress_data_range(True, [arch], [out.view(torch.bfloat16)], [0], [1])
        with pytest.raises(RuntimeError):
            dg.decompress_data_slice(False, [arch], [0], [16])
        with pytest.raises(RuntimeError):
            dg.decompress_data_slice(True, [arch], [0], [16], dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            distributed.decompress_shard(True, [arch], 0, 4)
        # lists of unequal length
        with pytest.raises(RuntimeError):
            dg.decompress_data_range(False, [arch, arch], [out], [0, 0], [1, 1])
        with pytest.raises(RuntimeError):
            dg.decompress_data_range(False, [arch], [out], [0, 0], [1])
        with pytest.raises(RuntimeError):
            dg.decompress_data_range(False, [arch], [out], [0], [1, 1])
        with pytest.raises(RuntimeError):
            dg.decompress_data_slice(False, [arch], [0, 1], [16])
        with pytest.raises(RuntimeError):
            dg.decompress_data_slice(False, [arch], [0], [16, 16])
        with pytest.raises(RuntimeError):
            dg.decompress_data_range(False, [], [], [], [])
        with pytest.raises(RuntimeError):
            dg.decompress_data_slice(False, [], [], [])
        # negative starts (and counts)
        with pytest.raises(RuntimeError):
            dg.decompress_data_slice(False, [arch], [-1], [16])
        with pytest.raises(RuntimeError):
            dg.decompress_data_slice(False, [arch], [0], [-16])
        with pytest.raises(RuntimeError):
            dg.decompress_data_range(False, [arch], [out], [-1], [1])
        # a dtype that is not one of the three float types
        for bad in (torch.float64, torch.int16, torch.uint8):
            with pytest.raises(RuntimeError):
                dg.decompress_data_slice(True, [arch], [0], [16], dtype=bad)
        with pytest.raises(RuntimeError):
            dg.decompress_data_slice(False, [arch], [0], [16], dtype=torch.float16)
    finally:
        dg.prefer_torch_ops(True)
