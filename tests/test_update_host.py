"""Decode-update without a GPU (dgpu_float_decode_update): the entry point is exported and bound, every invalid argument
is refused with DGPU_ERR_INVALID_ARGUMENT and a text before anything is enqueued (no call here reaches a device), the
empty batch returns 0, the argument checks of ops.decompress_data_update raise RuntimeError, and the declaration has no
temp-memory parameters."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dgpu_float_decode_update"


def _declaration():
    text = open(os.path.join(ROOT, "include", "dietgpu_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    (params,) = re.findall(r"\b%s\s*\(([^;{]*?)\)\s*;" % NAME, text, flags=re.S)
    return params


def test_the_declaration_has_no_temp_memory_parameters():
    params = _declaration()
    for name in ("temp_dev", "tempBytes", "tempUsed"):
        assert not re.search(r"\b%s\b" % name, params), name
    names = [p.split()[-1].lstrip("*") for p in params.split(",")]
    assert names == ["floatType", "probBits", "accumulate", "numInBatch", "in", "inBytes", "out", "outCapacity", "scale", "scale_dev",
                     "scaleStride", "seed", "seed_dev", "firstMember", "outSuccess_dev", "outSize_dev", "stream"]
    header = open(os.path.join(ROOT, "include", "dietgpu_amd.h")).read()
    doc = header[header.index("---- decode-update"): header.index("int " + NAME)]
    assert "No temp memory is used" in doc
    assert "#define DGPU_ABI_VERSION 8u" in header and NAME in header[: header.index("#define DGPU_ABI_VERSION")]


def test_entry_point_is_exported_and_bound():
    import dietgpu_amd
    from dietgpu_amd import distributed

    raw = ctypes.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    assert NAME in dietgpu_amd.EXPORTED_SYMBOLS and hasattr(raw, NAME)
    assert len(getattr(L, NAME).argtypes) == 17 and getattr(L, NAME).restype is ctypes.c_int
    assert callable(dietgpu_amd.decompress_data_update)
    assert list(inspect.signature(distributed.GpuFloatCodec.decompress_update).parameters) == [
        "self", "rows", "outs", "accumulate", "scale", "seed", "first_member"]
    assert "out_seed" in inspect.signature(distributed.compressed_all_reduce).parameters
    assert "same on every rank" in distributed.compressed_all_reduce.__doc__.lower()


def test_argument_errors_of_the_c_abi_need_no_device():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    f = getattr(L, NAME)
    one = (ctypes.c_uint32 * 1)(16)
    ptr = (ctypes.c_void_p * 1)(4096)
    dummy = ctypes.c_void_p(4096)  # a "device" address that is never followed: every call below fails before a launch

    def fails(message, ft=2, P=10, accumulate=1, n=1, ins=ptr, in_bytes=one, outs=ptr, caps=one, scale=0.5, scale_dev=None, stride=0,
              seed=1, seed_dev=None):
        assert f(ft, P, accumulate, n, ins, in_bytes, outs, caps, scale, scale_dev, stride, seed, seed_dev, 0, None, None, None) == 1
        text = L.dgpu_last_error().decode()
        assert message in text and text, text

    fails("floatType", ft=3)            # DGPU_FLOAT32 is rejected
    fails("floatType", ft=0)
    fails("floatType", ft=4)
    fails("probBits must be 9, 10 or 11", P=8)
    fails("probBits must be 9, 10 or 11", P=12)
    fails("numInBatch must be <= 65535", n=65536)
    fails("accumulate must be 0 or 1", accumulate=2)
    fails("accumulate must be 0 or 1", accumulate=-1)
    fails("scaleStride", scale_dev=dummy, stride=2)
    fails("scaleStride", stride=7)
    for bad in (0.0, -0.0, float("inf"), float("-inf"), float("nan")):
        fails("finite and not zero", scale=bad)
    fails("scale_dev must be 4-byte aligned", scale_dev=ctypes.c_void_p(4098))
    fails("seed_dev must be 8-byte aligned", seed_dev=ctypes.c_void_p(4100))
    for missing in ("ins", "in_bytes", "outs", "caps"):
        fails("null array", **{missing: None})
        fails("null array", scale=0.0, scale_dev=dummy, stride=1, **{missing: None})  # (a host scale is not looked at beside a device one)
    fails("16-byte aligned", ins=(ctypes.c_void_p * 1)(4096 + 8))
    fails("2-byte aligned", outs=(ctypes.c_void_p * 1)(8193))
    fails("outCapacity", caps=(ctypes.c_uint32 * 1)(0xFFFFF001))
    # an empty batch is fine
    assert f(2, 10, 1, 0, None, None, None, None, 0.5, None, 0, 1, None, 0, None, None, None) == 0
    assert f(1, 9, 0, 0, None, None, None, None, 0.0, dummy, 1, 2**64 - 1, dummy, 2**32 - 1, None, None, None) == 0


@pytest.mark.parametrize("torch_ops", [True, False])
def test_rejects_bad_arguments_without_a_gpu(torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        arch = torch.zeros(1024, dtype=torch.uint8)  # CPU tensors
        out = torch.zeros(4096, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            dg.decompress_data_update([arch], [out], 1)
        with pytest.raises(RuntimeError):
            dg.decompress_data_update([arch, arch], [out], 1)
        with pytest.raises(RuntimeError):
            dg.decompress_data_update([], [], 1)
        for bad in (-1, 2**64, 1.5, True, None, "seed"):
            with pytest.raises(RuntimeError, match="seed must be"):
                dg.decompress_data_update([arch], [out], bad)
        for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.float32)):
            with pytest.raises(RuntimeError, match="1-element int64"):
                dg.decompress_data_update([arch], [out], bad)
        with pytest.raises(RuntimeError, match="on the tensors' GPU"):  # a CPU seed tensor
            dg.decompress_data_update([arch], [out], torch.zeros(1, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="float32"):  # a scale of another dtype
            dg.decompress_data_update([arch], [out], 1, torch.ones(1, dtype=torch.float64))
        for wrong in (0, 2, 3):
            with pytest.raises(RuntimeError, match="1 element or one per archive"):
                dg.decompress_data_update([arch], [out], 1, torch.ones(wrong, dtype=torch.float32))
        for bad in (0.0, float("inf"), float("-inf"), float("nan"), 1e-60):
            with pytest.raises(RuntimeError, match="finite and not zero"):
                dg.decompress_data_update([arch], [out], 1, bad)
        for bad in (-1, 2**32, 0.5):
            with pytest.raises(RuntimeError, match="first_member"):
                dg.decompress_data_update([arch], [out], 1, first_member=bad)
    finally:
        dg.prefer_torch_ops(True)
