"""The stochastic rounding of the decode-update as the contract states it (include/dietgpu_amd.h,
dgpu_float_decode_update), on the CPU: the literals, the properties of `sround`, the torch restatement
(dietgpu_amd/rounding.py) against the numpy one (tests/sr_ref.py) bit for bit, and the statistics of the specification --
unbiased, and without correlation along the tensor, between seeds or between members.  Every statistical bound is 5
standard deviations of the quantity under the hypothesis that the decisions are independent with the stated
probabilities; with the rule of the contract every one of them stays within 4."""
import numpy as np
import pytest
import torch

import cast_ref as R
import sr_ref as S

FTS = (S.FLOAT16, S.BFLOAT16)
DTYPE = {S.FLOAT16: torch.float16, S.BFLOAT16: torch.bfloat16}
N = 98304
SEEDS = (0, 1, 0x0123456789ABCDEF, 2**64 - 1)
MEMBERS = (0, 1, 65534)
R_EDGES = (0, 1, 0x7FFF, 0x8000, 0xFFFF)


def _random_bits():
    rng = np.random.default_rng(11)
    return np.concatenate([R.EDGE_BITS, rng.integers(0, 2**32, 200000, dtype=np.uint64).astype(np.uint32)])


def test_the_literals():
    for s, j, key, rs in S.R16_LITERALS:
        assert S.member_key(s, j) == key, (hex(s), j)
        assert S.r16(s, j, S.R16_K).tolist() == rs, (hex(s), j)
    for table, ft in ((S.SROUND_BF16, S.BFLOAT16), (S.SROUND_FP16, S.FLOAT16)):
        for x, r, q in table:
            assert int(S.sround(np.array([x], dtype=np.uint32), r, ft)[0]) == q, (ft, hex(x), hex(r))
    for ft, t, w, f, v, qs in S.END_TO_END:
        n = len(qs)
        words, tensor = np.full(n, w, dtype=np.uint16), np.full(n, t, dtype=np.uint16)
        assert S.value(words, ft, f, tensor).tolist() == [v] * n
        assert S.update_ref(words, ft, f, 0, 0, tensor).tolist() == qs


@pytest.mark.parametrize("ft", FTS)
def test_a_representable_value_never_moves(ft):
    words = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    keep = ~S.is_nan16(words, ft)
    for r in R_EDGES:
        assert np.array_equal(S.sround(R.widen(words, ft), r, ft)[keep], words[keep]), (ft, r)
    nan = S.sround(R.widen(words, ft), 0, ft)[~keep]
    assert set(nan.tolist()) == ({0x7E00, 0xFE00} if ft == S.FLOAT16 else {0x7FC0, 0xFFC0})


@pytest.mark.parametrize("ft", FTS)
def test_sround_is_monotone_in_r_and_returns_truncation_or_one_unit_more(ft):
    bits = _random_bits()
    trunc = S.sround(bits, 0, ft).astype(np.int64)
    prev = trunc
    rs = sorted(set(R_EDGES) | set(range(0, 0x10000, 0x0555)) | {7, 8, 0xFFF8})
    for r in rs:
        q = S.sround(bits, r, ft).astype(np.int64)
        assert ((q == trunc) | (q == trunc + 1)).all(), (ft, r)   # (the sign bit is above: + 1 is one unit away from zero)
        assert (q >= prev).all(), (ft, r)
        prev = q
    # the largest r rounds every value with a remainder away from zero; none without one (bf16: 16 dropped bits; fp16
    # normal results: the top 13 of them decide with r >> 3)
    a = bits & 0x7FFFFFFF
    if ft == S.BFLOAT16:
        has = ((bits & 0xFFFF) != 0) & (a < 0x7F800000)
        assert np.array_equal(S.sround(bits, 0xFFFF, ft).astype(np.int64) == trunc + 1, has)


@pytest.mark.parametrize("ft", FTS)
def test_the_torch_restatement_equals_the_numpy_one(ft):
    from dietgpu_amd import rounding as T

    bits = _random_bits()
    rng = np.random.default_rng(12)
    r = rng.integers(0, 0x10000, len(bits)).astype(np.uint32)
    r[: len(R_EDGES)] = R_EDGES
    got = T.sround(torch.from_numpy(bits.astype(np.int64)), torch.from_numpy(r.astype(np.int64)), DTYPE[ft])
    assert np.array_equal(got.numpy().astype(np.uint16), S.sround(bits, r, ft))
    k = np.concatenate([np.arange(5000), np.array(S.R16_K), rng.integers(0, 2**32 - 4096, 5000)]).astype(np.int64)
    for s in SEEDS:
        for j in MEMBERS:
            assert int(T.member_key(s, j)) == S.member_key(s, j)
            seed = s if j else torch.tensor([s - 2**64 if s >= 2**63 else s], dtype=torch.int64)  # (an int, or its bits in a tensor)
            assert np.array_equal(T.r16(seed, j, torch.from_numpy(k)).numpy().astype(np.uint32), S.r16(s, j, k))
    # the whole update, in place, at a word offset
    words = R.cast_ref(rng.standard_normal(4097).astype(np.float32).view(np.uint32), ft)
    tensor = R.cast_ref(rng.standard_normal(4097).astype(np.float32).view(np.uint32), ft)
    for accumulate in (True, False):
        out = torch.from_numpy(tensor.view(np.int16).copy()).view(DTYPE[ft])
        product = torch.from_numpy(S.value(words, ft, -0.25).view(np.float32).copy())
        T.update_(out, product, SEEDS[2], 3, accumulate, first=8192)
        want = S.sround(S.value(words, ft, -0.25, tensor if accumulate else None), S.r16(SEEDS[2], 3, 8192 + np.arange(4097)), ft)
        assert np.array_equal(out.view(torch.int16).numpy().view(np.uint16), want), (ft, accumulate)


def _unit_and_fraction(v_bits, ft):
    """for finite float32 values: truncation toward zero to ft (as float64), the unit there, the remainder / unit"""
    t = S.sround(v_bits, 0, ft)
    up = (t.astype(np.uint32) + 1).astype(np.uint16)
    lo = R.widen(t, ft).view(np.float32).astype(np.float64)
    hi = R.widen(up, ft).view(np.float32).astype(np.float64)
    v = v_bits.view(np.float32).astype(np.float64)
    unit = np.abs(hi - lo)
    return lo, hi, unit, np.abs(v - lo) / unit


@pytest.mark.parametrize("member", MEMBERS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("ft", FTS)
def test_the_round_up_probability_is_the_remainder(ft, seed, member):
    """constant tensors with remainder 1/2, 1/4 and 1/8 of a unit: round-up counts within 5 binomial standard deviations;
    N(0,1) data: the summed error within 5 standard deviations of zero"""
    k = np.arange(N)
    r = S.r16(seed, member, k)
    one = 0x3F800000
    step = 0x10000 if ft == S.BFLOAT16 else 0x2000   # one unit of ft at 1.0, in float32 bits
    for f in (0.5, 0.25, 0.125):
        x = np.full(N, one + int(step * f), dtype=np.uint32)
        q = S.sround(x, r, ft).astype(np.int64)
        ups = int((q == int(S.sround(x[:1], 0, ft)[0]) + 1).sum())
        z = (ups - N * f) / np.sqrt(N * f * (1 - f))
        print(f"ft={ft} seed={seed:#x} member={member} remainder {f}: {ups} of {N} up, z = {z:+.2f}")
        assert abs(z) <= 5, (ft, seed, member, f, z)
    v = np.random.default_rng(7).standard_normal(N).astype(np.float32).view(np.uint32)
    lo, hi, unit, frac = _unit_and_fraction(v, ft)
    q = R.widen(S.sround(v, r, ft), ft).view(np.float32).astype(np.float64)
    assert ((q == lo) | (q == hi)).all()
    z = (q - v.view(np.float32).astype(np.float64)).sum() / np.sqrt((unit**2 * frac * (1 - frac)).sum())
    print(f"ft={ft} seed={seed:#x} member={member} N(0,1): z = {z:+.2f}")
    assert abs(z) <= 5, (ft, seed, member, z)


def _decisions(seed, member):
    """the +-1 decisions at remainder 1/2 (bf16: r >= 0x8000 rounds up)"""
    return np.where(S.r16(seed, member, np.arange(N)) >= 0x8000, 1.0, -1.0)


@pytest.mark.parametrize("member", MEMBERS)
@pytest.mark.parametrize("seed", SEEDS)
def test_the_decisions_are_not_autocorrelated(seed, member):
    d = _decisions(seed, member)
    for lag in (1, 2, 3, 64):
        c = float((d[:-lag] * d[lag:]).mean())
        print(f"seed={seed:#x} member={member} lag {lag}: {c * np.sqrt(N):+.2f} / sqrt(n)")
        assert abs(c) <= 5 / np.sqrt(N), (seed, member, lag, c)


def test_seeds_and_members_are_not_correlated_with_each_other():
    for what, ds in (("seeds", [_decisions(s, 0) for s in range(8)]), ("members", [_decisions(5, j) for j in range(8)])):
        for a in range(8):
            for b in range(a + 1, 8):
                c = float((ds[a] * ds[b]).mean())
                assert abs(c) <= 5 / np.sqrt(N), (what, a, b, c * np.sqrt(N))
