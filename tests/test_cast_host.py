"""Cast-compress, the parts that need no GPU: the conversion's reference (tests/cast_ref.py) against torch's CPU cast on
every non-NaN input and against literals on NaN, the C ABI entry point being exported and bound, its argument checks
(code 1 and the literal message, before anything touches a device) and those of the Python layer."""
import ctypes as C

import numpy as np
import pytest
import torch

import cast_ref as R

A = 0x10000  # a fake device address, aligned to everything
TOO_LARGE = 1717538816 + 1
NAME = "dgpu_float_cast_compress"
_TORCH = {R.BFLOAT16: torch.bfloat16, R.FLOAT16: torch.float16}


def _torch_cast(bits, ft):
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int32)).view(torch.float32)
    return t.to(_TORCH[ft]).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("ft", [R.BFLOAT16, R.FLOAT16])
def test_reference_conversion_equals_torch_on_every_non_nan_input(ft):
    rng = np.random.default_rng(2024)
    bits = np.concatenate([R.EDGE_BITS, rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)])
    finite = bits[(bits & 0x7FFFFFFF) <= 0x7F800000]
    assert finite.size > (1 << 20) * 0.99
    got, want = R.cast_ref(finite, ft), _torch_cast(finite, ft)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(finite[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    # the widened result rounds to itself
    assert (R.cast_ref(R.widen(got, ft), ft) == got).all()


def test_reference_conversion_literals():
    for bits, bf16, fp16 in R.LITERALS:
        assert int(R.cast_ref([bits], R.BFLOAT16)[0]) == bf16, hex(bits)
        assert int(R.cast_ref([bits], R.FLOAT16)[0]) == fp16, hex(bits)
    # every NaN of the edge table: canonical, sign kept, never an infinity
    nan = R.EDGE_BITS[(R.EDGE_BITS & 0x7FFFFFFF) > 0x7F800000]
    assert nan.size >= 14
    sign = ((nan >> 16) & 0x8000).astype(np.uint16)
    assert (R.cast_ref(nan, R.BFLOAT16) == (sign | 0x7FC0)).all()
    assert (R.cast_ref(nan, R.FLOAT16) == (sign | 0x7E00)).all()


def test_cast_entry_point_is_exported_and_bound():
    import dietgpu_amd

    raw = C.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    assert NAME in dietgpu_amd.EXPORTED_SYMBOLS and hasattr(raw, NAME)
    assert getattr(L, NAME).argtypes is not None and getattr(L, NAME).restype is C.c_int
    assert L.dgpu_abi_version() == 8  # an added entry point does not move the version
    assert callable(dietgpu_amd.compress_data_cast)
    from dietgpu_amd import distributed

    assert callable(distributed.compressed_all_reduce) and callable(distributed.GpuFloatCodec.compress_cast)


def _call(n=1, floatType=2, probBits=10, inp=None, sizes=None, out=None):
    import dietgpu_amd

    L = dietgpu_amd.lib()
    used = C.c_size_t(77)
    inp = (C.c_void_p * max(n, 1))(*(inp if inp is not None else [A] * n))
    out = (C.c_void_p * max(n, 1))(*(out if out is not None else [A] * n))
    sizes = (C.c_uint32 * max(n, 1))(*(sizes if sizes is not None else [4096] * n))
    rc = getattr(L, NAME)(None, 0, C.byref(used), floatType, probBits, n, inp, sizes, out, None, None)
    return rc, L.dgpu_last_error().decode(), used.value


@pytest.mark.parametrize("over,message", [
    (dict(floatType=0), "floatType of a cast archive must be float16 or bfloat16"),
    (dict(floatType=3), "floatType of a cast archive must be float16 or bfloat16"),
    (dict(floatType=4), "floatType of a cast archive must be float16 or bfloat16"),
    (dict(n=2, inp=[A, A + 2]), "float32 input must be 4-byte aligned"),
    (dict(n=2, inp=[A + 1, A]), "float32 input must be 4-byte aligned"),
    (dict(n=2, out=[A, A + 8]), "compressed output must be 16-byte aligned"),
    (dict(probBits=8), "probBits must be 9, 10 or 11"),
    (dict(probBits=12), "probBits must be 9, 10 or 11"),
    (dict(n=65536), "numInBatch must be <= 65535"),
    (dict(sizes=[TOO_LARGE]), "tensor larger than 1717538816 words: the maximum compressed size of its exponent plane exceeds INT32_MAX "
                              "(GpuANSEncode.cu:22)"),
])
def test_one_fault_gives_this_code_and_text(over, message):
    rc, text, _ = _call(**over)
    assert (rc, text) == (1, message)  # DGPU_ERR_INVALID_ARGUMENT


def test_sources_at_every_word_offset_pass_the_alignment_check():
    # (an empty batch ends after the checks; a batch of one would go on to the device)
    for ft in (1, 2):
        rc, _, used = _call(n=0, floatType=ft)
        assert rc == 0 and used == 0


@pytest.mark.parametrize("torch_ops", [True, False])
def test_ops_reject_bad_tensors_without_a_gpu(torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        x = torch.zeros(4096, dtype=torch.float32)  # a CPU tensor
        with pytest.raises(RuntimeError):
            dg.compress_data_cast([x], torch.bfloat16)
        with pytest.raises(RuntimeError):
            dg.compress_data_cast([], torch.bfloat16)
        for bad in (torch.float32, torch.float64, torch.int16, None):
            with pytest.raises(RuntimeError):
                dg.compress_data_cast([x], bad)
        for bad in (torch.bfloat16, torch.float16, torch.float64, torch.int32):
            with pytest.raises(RuntimeError):
                dg.compress_data_cast([x.to(bad)], torch.bfloat16)
    finally:
        dg.prefer_torch_ops(True)
