"""Reference of the feedback cast-compress call (include/dietgpu_amd.h, dgpu_float_feedback_compress), on float32 bits
with numpy, on top of tests/cast_ref.py:

  1. v = x + e, one IEEE float32 add (round to nearest even, denormals kept) -- or x itself, untouched, without a residual;
  2. q = cast_ref(v);
  3. e' = v - widen(q) where q is finite (exact), bits 0 where q is an infinity or a NaN;
  4. the archive is that of the float32 tensor v.

(-0) - (-0) is +0 in round to nearest, on the host as on the GPU: a fresh step of -0.0f leaves the residual bits
0x00000000 (pinned by LITERALS).  Where x and e are both NaN, or the add is invalid (inf - inf), IEEE leaves the sign of the
NaN open and so does the contract: `unambiguous` clears such pairs from random test data."""
import numpy as np

from cast_ref import BFLOAT16, FLOAT16, cast_ref, widen  # noqa: F401


def _f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def feedback_ref(x_bits, e_bits, ft):
    """uint32 bits of x and of the residual (None: no residual yet) -> (words q, new residual bits, v's bits)"""
    x = np.ascontiguousarray(x_bits, dtype=np.uint32)
    with np.errstate(all="ignore"):
        v = x.copy() if e_bits is None else (_f32(x) + _f32(e_bits)).view(np.uint32)
        q = cast_ref(v, ft)
        w = widen(q, ft)
        err = (_f32(v) - _f32(w)).view(np.uint32)
    finite = (w & 0x7F800000) != 0x7F800000
    return q, np.where(finite, err, 0).astype(np.uint32), v


def is_nan(bits):
    return (np.asarray(bits, dtype=np.uint32) & 0x7FFFFFFF) > 0x7F800000


def unambiguous(x_bits, e_bits):
    """e with the words changed whose sum's NaN sign IEEE leaves open: a NaN against a NaN (e becomes 1.0f) and an
    infinity against the opposite infinity (e becomes 0)"""
    x = np.asarray(x_bits, dtype=np.uint32)
    e = np.array(e_bits, dtype=np.uint32)
    e[is_nan(x) & is_nan(e)] = 0x3F800000
    inf = lambda b: (b & 0x7FFFFFFF) == 0x7F800000
    e[inf(x) & inf(e) & ((x ^ e) >> 31 == 1)] = 0
    return e


# (x, e or None, float type, v or None, q or None, e' or None): the rows the contract states as literals
# (1 + 2^-8 is a tie between two bfloat16 words and goes to the even one, 1.0: half a unit of the last place, 2^-8 =
# 0x3B800000, is left over -- and comes back, whole, when it is added to 1.0 in the next step)
LITERALS = [
    (0x3F808000, 0x00000000, BFLOAT16, 0x3F808000, 0x3F80, 0x3B800000),
    (0x3F800000, 0x3B800000, BFLOAT16, 0x3F808000, 0x3F80, 0x3B800000),
    (0x7F7F8000, 0x00000000, BFLOAT16, None, 0x7F80, 0x00000000),
    (0x477FF000, 0x00000000, FLOAT16, None, 0x7C00, 0x00000000),
    (0x7FC00000, 0x00000000, BFLOAT16, None, 0x7FC0, 0x00000000),
    (0x7FC00000, 0x3F800000, FLOAT16, None, 0x7E00, 0x00000000),
    (0x7FC00000, 0x7F800000, BFLOAT16, None, 0x7FC0, 0x00000000),
    # -0 without a residual keeps its sign in q; (-0) - (-0) = +0: the residual is bits 0
    (0x80000000, None, BFLOAT16, 0x80000000, 0x8000, 0x00000000),
    (0x80000000, None, FLOAT16, 0x80000000, 0x8000, 0x00000000),
    # ... and with a zero residual the add has made it +0
    (0x80000000, 0x00000000, BFLOAT16, 0x00000000, 0x0000, 0x00000000),
    (0x80000000, 0x00000000, FLOAT16, 0x00000000, 0x0000, 0x00000000),
]
