"""Inputs and expected values of the decode-reduce tests: S sources per accumulator, built on the cases of
tests/accum_cases.py.  Source 0 of a member is the case's own element; source s has the same word count, the kinds of
its whole blocks rotated by s (so that within one tile some sources stage whole and others take the ring) and another
seed.  The expected value is `accum_cases.add` applied source by source, left to right.

This module touches no GPU state: it is imported by tests that run without one."""
import functools

import numpy as np

import accum_cases as C
import oracle as O

MAX_SOURCES = 8


def rotated(kinds, s):
    s %= max(len(kinds), 1)
    return kinds[s:] + kinds[:s]


def reduce_expected(start, wides, accumulate):
    """((start + x0) + x1) + ... with accumulate, (x0 + x1) + ... without (x0 as it is): one float32 add per source"""
    acc = start if accumulate else None
    for w in wides:
        acc = w.astype(np.float32) if acc is None else C.add(acc, w)
    return acc


def finite_bits(n, seed):
    """a random bit pattern per float32 word, every one finite (an all-ones exponent has its lowest bit cleared): a sum
    with it may overflow to +-inf but is never NaN, so it compares bit for bit"""
    rng = np.random.default_rng([77, seed])
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    w[(w & 0x7F800000) == 0x7F800000] &= np.uint32(0xFF7FFFFF)
    return w.view(np.float32)


def any_bits(n, seed):
    """a truly random bit pattern per word, NaN payloads and infinities included: for accumulators that must not change"""
    return np.random.default_rng([78, seed]).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


class Sources:
    """`sources` sources for every element of an accum_cases.Case"""

    def __init__(self, case, sources):
        self.case, self.ft, self.S = case, case.ft, sources
        self.sizes = case.sizes
        self.words = [list(case.words)]
        for s in range(1, sources):
            row = []
            for i, n in enumerate(case.sizes):
                whole, tail = n // C.BLK, n % C.BLK
                kinds = case.kinds[i][:whole]
                tail_kind = case.kinds[i][-1] if tail else "c"
                row.append(C.words(case.ft, rotated(kinds, s), tail, tail_kind, seed=900000 + 7919 * s + 31 * i + len(case.tag)))
            self.words.append(row)

    @functools.cached_property
    def wide(self):  # [source][element]
        return [[C.widen(self.ft, w) for w in row] for row in self.words]

    @functools.lru_cache(maxsize=None)
    def archives(self, prob_bits):  # [source][element]
        first = self.case.archives(prob_bits)
        return [first] + [[O.float_compress(self.ft, w, prob_bits) for w in row] for row in self.words[1:]]

    @functools.cached_property
    def start(self):
        return self.case.start

    @functools.lru_cache(maxsize=None)
    def expected(self, sources, accumulate, reps=1):
        """per element: the first `sources` sources summed in order, onto `start` if accumulate; `reps` times over"""
        out = []
        for i in range(len(self.sizes)):
            acc = self.start[i]
            for _ in range(reps):
                acc = reduce_expected(acc, [self.wide[s][i] for s in range(sources)], accumulate)
            out.append(acc)
        return out


@functools.lru_cache(maxsize=None)
def staging(ft):
    return Sources(C.staging(ft, 0), MAX_SOURCES)


@functools.lru_cache(maxsize=None)
def tails(ft, lead):
    return Sources(C.tails(ft, lead), 2)


@functools.lru_cache(maxsize=None)
def orders(ft, B, tile_blocks):
    return Sources(C.orders(ft, B, tile_blocks), 2)


@functools.lru_cache(maxsize=None)
def malformed(ft, name):
    return Sources(C.malformed(ft, name), 3)


# the order test: three values, exact in fp16, bf16 and fp32, whose float32 sum depends on the order
ORDER_VALUES = (2.0 ** 15, -(2.0 ** 15), 2.0 ** -10)
ORDER_WORDS = 5 * C.BLK + 123


def constant_words(ft, value, n=ORDER_WORDS):
    """n words of `ft` that all hold `value` (which the type represents exactly)"""
    import torch

    t = torch.full((n,), value, dtype=torch.float32).to(C.DTYPE[ft])
    assert float(t[0].to(torch.float32)) == value
    return np.ascontiguousarray(t.view(torch.int16 if ft != O.FLOAT32 else torch.int32).numpy().view(C.WORD[ft]))
