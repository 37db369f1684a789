"""The stochastic rounding of the decode-update (include/dietgpu_amd.h, dgpu_float_decode_update), restated from the
contract with integer arithmetic on the bits: `sround` (float32 bits and a 16-bit number -> a word of float16 / bfloat16),
`r16` (seed, member, word index -> the 16-bit number) and the three-step update (one numpy float32 multiply, one numpy
float32 add, sround).  Builds on cast_ref.widen.  The reference of tests/test_update_ref_host.py, tests/test_gpu_update.py
and the 16-bit-output tests of the collectives.  Touches no GPU state."""
import numpy as np

import cast_ref as R

FLOAT16, BFLOAT16 = 1, 2
_M32 = np.uint64(0xFFFFFFFF)


def mix32(x):
    """uint32 array (held in uint64) -> uint32 array (held in uint64)"""
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def member_key(seed, member):
    """key_j of (S, j) -> int"""
    seed, member = int(seed), int(member)
    assert 0 <= seed < (1 << 64) and 0 <= member < (1 << 32)
    base = int(mix32(int(mix32(((seed & 0xFFFFFFFF) + 0x9E3779B9) & 0xFFFFFFFF)) ^ (seed >> 32)))
    return int(mix32((base + member * 0x85EBCA6B) & 0xFFFFFFFF))


def r16(seed, member, k):
    """the 16-bit numbers of words k (an array of word indices) of member `member` under `seed` -> uint32 array"""
    k = np.asarray(k, dtype=np.uint64)
    bits = mix32(np.uint64(member_key(seed, member)) ^ (k >> np.uint64(1)))
    return np.where(k & np.uint64(1), bits >> np.uint64(16), bits & np.uint64(0xFFFF)).astype(np.uint32)


def sround(bits, r, ft):
    """float32 bits (uint32) and 16-bit numbers r -> uint16 words of float type `ft`"""
    x = np.ascontiguousarray(bits, dtype=np.uint32).astype(np.uint64)
    r = np.broadcast_to(np.asarray(r, dtype=np.uint64), x.shape)
    assert int(r.max(initial=0)) <= 0xFFFF
    a = x & np.uint64(0x7FFFFFFF)
    sign = (x >> np.uint64(16)) & np.uint64(0x8000)
    nan = a > np.uint64(0x7F800000)
    if ft == BFLOAT16:
        q = ((x + r) >> np.uint64(16)) & np.uint64(0xFFFF)
        return np.where(nan, sign | np.uint64(0x7FC0), q).astype(np.uint16)
    assert ft == FLOAT16
    e = a >> np.uint64(23)
    m = (a & np.uint64(0x7FFFFF)) | np.where(e != 0, np.uint64(0x800000), np.uint64(0))
    shift = np.uint64(113) - np.maximum(e, np.uint64(1)).clip(None, np.uint64(113))  # (e >= 113 takes the other branch)
    low = np.where(shift >= np.uint64(32), np.uint64(0), m >> np.minimum(shift, np.uint64(63)))
    u = np.where(a >= np.uint64(0x38800000), a - np.uint64(0x38000000), low)
    h = np.minimum((u + (r >> np.uint64(3))) >> np.uint64(13), np.uint64(0x7C00))
    return np.where(nan, sign | np.uint64(0x7E00), sign | h).astype(np.uint16)


def value(words, ft, factor, tensor=None):
    """steps 1 and 2: float32 bits of [widen(tensor) +] fl32(widen(word) * factor); tensor None: accumulate off"""
    with np.errstate(all="ignore"):
        p = (R.widen(words, ft).view(np.float32) * np.float32(factor)).astype(np.float32)
        if tensor is not None:
            p = (R.widen(tensor, ft).view(np.float32) + p).astype(np.float32)
    return np.ascontiguousarray(p).view(np.uint32).copy()


def update_ref(words, ft, factor, seed, member, tensor=None, first=0):
    """the words dgpu_float_decode_update leaves for archive words `words` (word indices first, first + 1, ...) -> uint16"""
    v = value(words, ft, factor, tensor)
    return sround(v, r16(seed, member, first + np.arange(len(v), dtype=np.uint64)), ft)


def is_nan16(words, ft):
    w = np.asarray(words, dtype=np.uint16)
    return (w & 0x7FFF) > (0x7F80 if ft == BFLOAT16 else 0x7C00)


def mask_nan_sign(words, ft):
    """the words with the sign of every NaN cleared (the sign of a NaN the arithmetic produced is unspecified)"""
    w = np.asarray(words, dtype=np.uint16)
    return np.where(is_nan16(w, ft), w & 0x7FFF, w).astype(np.uint16)


# ---- the literals of the contract -------------------------------------------------------------------------------
R16_K = [0, 1, 2, 3, 4097, 2**31 - 2]
#   (S, j, key, r16 at R16_K)
R16_LITERALS = [
    (0, 0, 0x944FB554, [0x9E5E, 0x41F3, 0x55BB, 0x2B4B, 0xE426, 0xE76F]),
    (1, 0, 0xD661FF16, [0x364E, 0xD3EC, 0x554C, 0x84EF, 0xBF2E, 0x1E0E]),
    (0, 1, 0x3A678045, [0x3F70, 0xED55, 0x51F8, 0x9BDC, 0xC356, 0x92E9]),
    (0x0123456789ABCDEF, 3, 0x826E1F73, [0xFFB2, 0x74E0, 0x4171, 0xB0CD, 0xB7C0, 0xA6D7]),
    (2**64 - 1, 65534, 0x2E75E58D, [0xB53E, 0xD6EC, 0xA07F, 0x44B4, 0x0980, 0xEA1C]),
]
#   (x, r, q)
SROUND_BF16 = [
    (0x3F808000, 0x7FFF, 0x3F80), (0x3F808000, 0x8000, 0x3F81), (0xBF808000, 0x8000, 0xBF81), (0x3F800001, 0xFFFF, 0x3F81),
    (0x3F800001, 0xFFFE, 0x3F80), (0x7F800000, 0xFFFF, 0x7F80), (0x7F7FFFFF, 0x0001, 0x7F80), (0x7F7FFFFF, 0x0000, 0x7F7F),
    (0x80000000, 0xFFFF, 0x8000), (0x00000001, 0xFFFF, 0x0001), (0xFF800001, 0x0000, 0xFFC0),
]
SROUND_FP16 = [
    (0x3F801000, 0x7FFF, 0x3C00), (0x3F801000, 0x8000, 0x3C01), (0x477FF000, 0x8000, 0x7C00), (0x477FF000, 0x7FFF, 0x7BFF),
    (0x477FE000, 0xFFFF, 0x7BFF), (0x47800000, 0x0000, 0x7C00), (0x33800000, 0xFFFF, 0x0001), (0x33000000, 0x7FFF, 0x0000),
    (0x33000000, 0x8000, 0x0001), (0x387FFFFF, 0x0000, 0x03FF), (0x387FFFFF, 0x0008, 0x0400), (0x00000001, 0xFFFF, 0x0000),
    (0x7F800001, 0x0000, 0x7E00), (0x80000000, 0xFFFF, 0x8000),
]
#   (ft, tensor word, archive word, factor, v, the words at k = 0, 1, ...) with S = 0, member 0, accumulate = 1
END_TO_END = [
    (BFLOAT16, 0x3F80, 0x3C00, -0.25, 0x3F7F8000, [0x3F80, 0x3F7F, 0x3F7F, 0x3F7F, 0x3F80, 0x3F80]),
    (FLOAT16, 0x3C00, 0x1000, 1.0, 0x3F801000, [0x3C01, 0x3C00, 0x3C00, 0x3C00]),
]
