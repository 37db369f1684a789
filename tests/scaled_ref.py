"""The arithmetic of the scaled decompress (include/dietgpu_amd.h, dgpu_float_decode_scaled), on the bits: the exact
widening of tests/cast_ref.py, ONE numpy float32 multiply (IEEE, round to nearest even, denormals kept) and ONE rounding
to the type by cast_ref.  The reference of tests/test_decode_scaled_host.py, tests/test_gpu_decode_scaled.py and the
clipping tests of the collectives.  Touches no GPU state."""
import numpy as np

import cast_ref as R

FLOAT16, BFLOAT16, FLOAT32 = 1, 2, 3


def f32(x):
    """a Python number rounded once to float32"""
    return np.float32(x)


def scaled_ref(words, ft, factor):
    """words of float type `ft` (uint16; uint32 for float32) times the float32 `factor` -> words of `ft`"""
    f = np.float32(factor)
    if ft == FLOAT32:
        wide = np.ascontiguousarray(words, dtype=np.uint32).view(np.float32)
    else:
        wide = R.widen(words, ft).view(np.float32)
    with np.errstate(all="ignore"):
        prod = (wide * f).astype(np.float32)
    bits = np.ascontiguousarray(prod).view(np.uint32)
    return bits.copy() if ft == FLOAT32 else R.cast_ref(bits, ft)


def is_nan(words, ft):
    w = np.asarray(words)
    if ft == FLOAT32:
        return (w & 0x7FFFFFFF) > 0x7F800000
    if ft == FLOAT16:
        return (w & 0x7FFF) > 0x7C00
    return (w & 0x7FFF) > 0x7F80


def is_inf(words, ft):
    w = np.asarray(words)
    if ft == FLOAT32:
        return (w & 0x7FFFFFFF) == 0x7F800000
    if ft == FLOAT16:
        return (w & 0x7FFF) == 0x7C00
    return (w & 0x7FFF) == 0x7F80
