"""The float32 -> float16 / bfloat16 conversion of the cast-compress path, defined on the bits with integer arithmetic
(include/dietgpu_amd.h, dgpu_float_cast_compress): round to nearest even, denormals kept, overflow to infinity, every
NaN to the canonical quiet NaN with its sign.  The reference of tests/test_cast_host.py and tests/test_gpu_cast.py."""
import numpy as np

FLOAT16, BFLOAT16 = 1, 2


def cast_ref(bits, ft):
    """uint32 float32 bits -> uint16 words of float type `ft`"""
    x = np.ascontiguousarray(bits, dtype=np.uint32).astype(np.uint64)
    sign = (x >> 16) & 0x8000
    a = x & 0x7FFFFFFF
    nan = a > 0x7F800000
    if ft == BFLOAT16:
        r = (x + 0x7FFF + ((x >> 16) & 1)) >> 16
        return np.where(nan, sign | 0x7FC0, r).astype(np.uint16)
    assert ft == FLOAT16
    # normal results (|v| >= 2^-14): rebias the exponent, round the 13 dropped bits; a carry runs into the exponent and,
    # from 65520 on, into infinity
    normal = np.minimum((a - 0x38000000 + 0xFFF + ((a >> 13) & 1)) >> 13, 0x7C00)
    # denormal results: the 24-bit significand shifted right by t = 126 - exponent bits (14 .. 25; below that, zero)
    t = np.minimum(126 - (a >> 23).astype(np.int64), 25).clip(14, 25).astype(np.uint64)
    m = (a & 0x7FFFFF) | 0x800000
    denormal = (m + (np.uint64(1) << (t - 1)) - 1 + ((m >> t) & 1)) >> t
    r = np.where(a >= 0x38800000, normal, denormal)
    return np.where(nan, sign | 0x7E00, sign | r).astype(np.uint16)


def widen(words, ft):
    """uint16 words of `ft` -> uint32 float32 bits, exact"""
    w = np.ascontiguousarray(words, dtype=np.uint16)
    if ft == BFLOAT16:
        return w.astype(np.uint32) << 16
    return w.view(np.float16).astype(np.float32).view(np.uint32)


# float32 bit patterns at every edge of the two conversions (positive; EDGE_BITS adds the negatives)
_EDGES = [
    0x00000000, 0x7F800000,                          # zero, infinity
    0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF,  # bf16 ties to even both ways, just above / below a tie
    0x3F801000, 0x3F803000, 0x3F801001, 0x3F800FFF,  # fp16 ties to even both ways, just above / below a tie
    0x3FFFFFFF, 0x3F7FFFFF, 0x3FFF8000, 0x3FFFF000,  # mantissa all ones: the carry runs into the exponent
    0x7F7F8000, 0x7F7FFFFF, 0x7F7F7FFF,              # bf16 overflow to infinity / the largest that stays finite
    0x477FF000, 0x477FEFFF, 0x477FE000, 0x47800000, 0x7F000000,  # fp16: 65520 -> inf, just below, 65504, 65536, huge
    0x38800000, 0x387FFFFF, 0x387FE000, 0x387FF000, 0x38000000,  # fp16 smallest normal, denormals and their carry
    0x33800000, 0x33000001, 0x33000000, 0x32FFFFFF, 0x33800001, 0x33C00000, 0x34000000,  # fp16 smallest denormal, ties, zero
    0x007FFFFF, 0x00008000, 0x00008001, 0x00018000, 0x00000001, 0x00400000,  # float32 denormal inputs
    0x7FC00000, 0x7FA00000, 0x7F800001, 0x7F80FFFF, 0x7FFFFFFF, 0x7F808001, 0x7FC12345,  # NaN: payload high, low, both
]
EDGE_BITS = np.array(_EDGES + [v | 0x80000000 for v in _EDGES], dtype=np.uint32)
# (bits, bf16, fp16) rows the issue states as literals
LITERALS = [
    (0x007FFFFF, 0x0080, 0x0000), (0x00008000, 0x0000, 0x0000), (0x00008001, 0x0001, 0x0000), (0x7F7F8000, 0x7F80, 0x7C00),
    (0x33000001, 0x3300, 0x0001), (0x33000000, 0x3300, 0x0000), (0x387FFFFF, 0x3880, 0x0400), (0x477FF000, 0x4780, 0x7C00),
    (0x477FEFFF, 0x4780, 0x7BFF), (0x80000000, 0x8000, 0x8000), (0x3FFFFFFF, 0x4000, 0x4000),
    (0x7F800001, 0x7FC0, 0x7E00), (0xFF800001, 0xFFC0, 0xFE00), (0x7FC00000, 0x7FC0, 0x7E00), (0xFFA00000, 0xFFC0, 0xFE00),
    (0x7FFFFFFF, 0x7FC0, 0x7E00), (0xFF80FFFF, 0xFFC0, 0xFE00), (0x7F800000, 0x7F80, 0x7C00), (0xFF800000, 0xFF80, 0xFC00),
]
