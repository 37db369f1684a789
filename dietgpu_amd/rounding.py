"""The stochastic rounding of dgpu_float_decode_update (include/dietgpu_amd.h) restated in torch on integer tensors: the
fall-back of the collectives for codecs without `decompress_update`, on any device (this module needs no ROCm and loads no
library).  Unsigned 32-bit quantities travel in int64 tensors; every function gives the bits the kernel gives.

    mix32(x):      x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (mod 2^32)
    r16(S, j, k):  base = mix32(mix32(lo32(S) + 0x9E3779B9) ^ hi32(S)); key = mix32(base + j * 0x85EBCA6B);
                   bits = mix32(key ^ (k >> 1)); the low half of bits for even k, the high half for odd k
    sround(x, r):  NaN -> the canonical quiet NaN with its sign; bfloat16: (x + r) >> 16; float16: u = |x| in units of 2^-13
                   of a float16 last place (floor), min((u + (r >> 3)) >> 13, 0x7c00) under the sign
"""
import torch

_M32 = 0xFFFFFFFF


def mix32(x):
    x = x & _M32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32  # (the int64 product wraps; its low 32 bits are exact)
    return x ^ (x >> 16)


def _seed_bits(seed, device):
    """an int in [0, 2^64) or a 1-element int64 tensor whose bits are the seed -> (lo32, hi32) as int64 tensors"""
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or seed.numel() != 1:
            raise RuntimeError("a tensor seed must be a 1-element int64 tensor")
        s = seed.reshape(()).to(device)
    else:
        if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < (1 << 64):
            raise RuntimeError("seed must be an int in [0, 2^64) or a 1-element int64 tensor")
        s = torch.tensor(seed - (1 << 64) if seed >= (1 << 63) else seed, dtype=torch.int64, device=device)
    return s & _M32, (s >> 32) & _M32


def member_key(seed, member, device="cpu"):
    """key_j of (S, j) -> a 0-dim int64 tensor"""
    if not 0 <= int(member) < (1 << 32):
        raise RuntimeError("member must be in [0, 2^32)")
    lo, hi = _seed_bits(seed, device)
    base = mix32(mix32(lo + 0x9E3779B9) ^ hi)
    return mix32(base + ((int(member) * 0x85EBCA6B) & _M32))


def r16(seed, member, k):
    """the 16-bit numbers of the words with indices k (an int64 tensor) of member `member` under `seed` -> int64 tensor"""
    bits = mix32(member_key(seed, member, k.device) ^ (k >> 1))
    return torch.where((k & 1) != 0, bits >> 16, bits & 0xFFFF)


def sround(bits, r, dtype):
    """float32 bits (int64 tensor of values in [0, 2^32)) and 16-bit numbers r -> the words of `dtype` (torch.bfloat16 or
    torch.float16) as an int64 tensor of values in [0, 2^16)"""
    x = bits & _M32
    a = x & 0x7FFFFFFF
    sign = (x >> 16) & 0x8000
    nan = a > 0x7F800000
    if dtype == torch.bfloat16:
        return torch.where(nan, sign | 0x7FC0, ((x + r) >> 16) & 0xFFFF)
    if dtype != torch.float16:
        raise RuntimeError("stochastic rounding: float16 or bfloat16")
    e = a >> 23
    m = (a & 0x7FFFFF) | torch.where(e != 0, 0x800000, 0)
    shift = (113 - e.clamp(1, 113)).clamp(max=32)  # (m < 2^24: a shift of 32 leaves 0; e >= 113 takes the other branch)
    u = torch.where(a >= 0x38800000, a - 0x38000000, m >> shift)
    h = ((u + (r >> 3)) >> 13).clamp(max=0x7C00)
    return torch.where(nan, sign | 0x7E00, sign | h)


def stochastic_round_(out, value, seed, member, first=0):
    """out[k] = sround(bits(value[k]), r16(seed, member, first + k)): `value` a float32 tensor, `out` a contiguous float16 or
    bfloat16 tensor of the same number of elements on the same device, written in place -> out"""
    if value.dtype != torch.float32 or out.dtype not in (torch.float16, torch.bfloat16) or not out.is_contiguous():
        raise RuntimeError("stochastic_round_: a float32 value and a contiguous float16 / bfloat16 output")
    if value.numel() != out.numel() or value.device != out.device:
        raise RuntimeError("stochastic_round_: value and out must have one size and one device")
    bits = value.contiguous().view(torch.int32).reshape(-1).to(torch.int64) & _M32
    k = torch.arange(first, first + bits.numel(), dtype=torch.int64, device=out.device)
    q = sround(bits, r16(seed, member, k), out.dtype)
    q = torch.where(q >= 0x8000, q - 0x10000, q).to(torch.int16)
    out.view(torch.int16).reshape(-1).copy_(q)
    return out


def update_(out, product, seed, member, accumulate=True, first=0):
    """steps 2 and 3 of dgpu_float_decode_update for a float32 `product` = fl32(widen(word) * s):
    out = sround([widen(out) +] product) -- ONE float32 add, then the stochastic rounding -> out"""
    v = out.to(torch.float32).reshape(-1) + product.reshape(-1) if accumulate else product.reshape(-1)
    return stochastic_round_(out, v, seed, member, first)
