"""The arithmetic of the scaled decode-accumulate (include/dietgpu_amd.h, dgpu_float_decode_accumulate_scaled), on the
bits: the exact widening of tests/cast_ref.py, ONE numpy float32 multiply and ONE numpy float32 add (IEEE, round to
nearest even, denormals kept, two roundings -- never a fused multiply-add), floating-point errors ignored.  The reference
of tests/test_accum_scaled_host.py, tests/test_gpu_accum_scaled.py and the float32-output tests of the collectives.
Touches no GPU state."""
import numpy as np

import cast_ref as R

FLOAT16, BFLOAT16, FLOAT32 = 1, 2, 3


def widen(words, ft):
    """words of float type `ft` (uint16; uint32 for float32) -> their exact float32 values"""
    if ft == FLOAT32:
        return np.ascontiguousarray(words, dtype=np.uint32).view(np.float32)
    return R.widen(words, ft).view(np.float32)


def product(words, ft, factor):
    """fl32(widen(word) * factor) -> float32 bits"""
    with np.errstate(all="ignore"):
        p = (widen(words, ft) * np.float32(factor)).astype(np.float32)
    return np.ascontiguousarray(p).view(np.uint32).copy()


def accum_scaled_ref(words, ft, factor, acc_bits=None):
    """float32 bits of [acc +] fl32(widen(word) * factor); acc_bits (uint32) None: accumulate off, the product is stored"""
    p = product(words, ft, factor)
    if acc_bits is None:
        return p
    a = np.ascontiguousarray(acc_bits, dtype=np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        s = (a + p.view(np.float32)).astype(np.float32)
    return np.ascontiguousarray(s).view(np.uint32).copy()


def is_nan(bits):
    return (np.asarray(bits, dtype=np.uint32) & 0x7FFFFFFF) > 0x7F800000
