"""The reference of stochastic cast-compress (include/dietgpu_amd.h, dgpu_float_stochastic_compress): the 16-bit words are
sr_ref.sround(bits, sr_ref.r16(seed, member, arange(n)), ft) -- the rounding and the random bits of the decode-update,
restated once in tests/sr_ref.py -- and the archive is the CPU oracle's float_compress of those words.  Touches no GPU
state."""
import numpy as np

import sr_ref as S

FLOAT16, BFLOAT16 = S.FLOAT16, S.BFLOAT16


def words(bits, ft, seed, member):
    """float32 bits of one member -> the uint16 words its archive holds"""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    return S.sround(bits, S.r16(seed, member & 0xFFFFFFFF, np.arange(bits.size, dtype=np.uint64)), ft)


def archive(bits, ft, seed, member, prob_bits=10):
    """-> (the archive's bytes, the words it holds)"""
    import oracle as O

    w = words(bits, ft, seed, member)
    return O.float_compress(ft, w, prob_bits), w
