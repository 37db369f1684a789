"""Inputs of the decode-accumulate and ranged-decode path tests, built block by block so that the decoder's staging
modes are chosen by the DATA: a wave stages its two blocks whole in LDS when both have <= 1024 compressed 16-bit words
and takes the 2 KiB word ring otherwise.  N(0, 1) inputs give every float type exactly one of the two modes.

A block is of one of three kinds, defined through the byte the float codec compresses (oracle.float_split /
float_join), so the same recipe works for all three float types:
  "c"  compressible: that byte drawn from 4 values with p = 0.7 / 0.2 / 0.07 / 0.03, every other bit random
  "r"  incompressible but finite: uniform random bit patterns; an all-ones exponent field has its lowest bit cleared
  "b"  boundary: 17 nearly equiprobable values k * 13 + 3 of that byte, a little over 4 bits per symbol: blocks of
       1024 words give or take a few (the recipe of test_decoder_staging_boundary)
Every word is finite, so a sum with a finite accumulator is never NaN (it may overflow to +-inf, which compares bit for
bit).  tests/test_accumulate_cases_host.py asserts these premises with the CPU oracle; the GPU tests import the same
cases, and decode oracle archives of them.

This module touches no GPU state: it is imported by tests that run without one.
"""
import functools
import zlib

import numpy as np
import torch

import oracle as O

BLK = 4096
STAGE_WORDS = 1024  # a block of up to this many compressed words can be staged whole (kRingBytes / 2)
FTS = (O.FLOAT16, O.BFLOAT16, O.FLOAT32)
PROB_BITS = (9, 10, 11)
WORD = {O.FLOAT16: np.uint16, O.BFLOAT16: np.uint16, O.FLOAT32: np.uint32}
SIGNED = {O.FLOAT16: np.int16, O.BFLOAT16: np.int16, O.FLOAT32: np.int32}
DTYPE = {O.FLOAT16: torch.float16, O.BFLOAT16: torch.bfloat16, O.FLOAT32: torch.float32}
EXP_MASK = {O.FLOAT16: 0x7C00, O.BFLOAT16: 0x7F80, O.FLOAT32: 0x7F800000}
EXP_LOW = {O.FLOAT16: 0x0400, O.BFLOAT16: 0x0080, O.FLOAT32: 0x00800000}
# the four values of the compressed byte of a "c" block: magnitudes around one, so that an add changes the accumulator
# (fp16: sign, exponent and two mantissa bits -- 1, -1, 0.5, 2; bf16 / fp32: the exponent)
C_BYTES = {O.FLOAT16: (0x3C, 0xBC, 0x38, 0x40), O.BFLOAT16: (127, 126, 128, 125), O.FLOAT32: (127, 126, 128, 125)}
C_P = (0.7, 0.2, 0.07, 0.03)
B_BYTES = np.arange(17, dtype=np.uint8) * 13 + 3  # 3 .. 211: finite in every type (fp16: not 0x7C..0x7F, < 0xF8)
_bp = np.array([1.3, 1.2, 1.1] + [1.0] * 11 + [0.9, 0.8, 0.7])
B_P = _bp / _bp.sum()


def _random_words(rng, ft, n):
    hi = 1 << (32 if ft == O.FLOAT32 else 16)
    return rng.integers(0, hi, n, dtype=np.uint64).astype(WORD[ft])


def _with_compressed_byte(ft, comp, rng):
    """words whose compressed byte is comp[i] and whose other bits are random"""
    n = comp.size
    _, rest = O.float_split(ft, _random_words(rng, ft, n))
    return O.float_join(ft, comp, rest, n).astype(WORD[ft])


def block(ft, kind, n, rng_byte, rng_rest):
    """n words of one kind; the compressed bytes of "c" and "b" come from rng_byte alone"""
    if kind == "c":
        comp = rng_byte.choice(np.array(C_BYTES[ft], np.uint8), n, p=C_P)
    elif kind == "b":
        comp = rng_byte.choice(B_BYTES, n, p=B_P)
    elif kind == "r":
        w = _random_words(rng_rest, ft, n)
        ones = (w & WORD[ft](EXP_MASK[ft])) == EXP_MASK[ft]
        w[ones] &= WORD[ft](~EXP_LOW[ft] & (0xFFFFFFFF if ft == O.FLOAT32 else 0xFFFF))
        return w
    else:
        raise ValueError(kind)
    return _with_compressed_byte(ft, comp, rng_rest)


def words(ft, kinds, tail=0, tail_kind="c", seed=0):
    """one element: a whole block per letter of `kinds`, then `tail` words of tail_kind.  The compressed bytes of "c" and
    "b" blocks depend on the seed only (a "b" element compresses to the same block sizes in every float type)."""
    rng_byte = np.random.default_rng([seed, 0])
    rng_rest = np.random.default_rng([seed, ft])
    parts = [block(ft, k, BLK, rng_byte, rng_rest) for k in kinds]
    if tail:
        parts.append(block(ft, tail_kind, tail, rng_byte, rng_rest))
    return np.ascontiguousarray(np.concatenate(parts), WORD[ft])


def finite(ft, w):
    return (w & WORD[ft](EXP_MASK[ft])) != EXP_MASK[ft]


def widen(ft, w):
    """the exact float32 value of every word: torch on the CPU"""
    return torch.from_numpy(w.view(SIGNED[ft]).copy()).view(DTYPE[ft]).to(torch.float32).numpy()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def add(acc, wide):
    """one IEEE float32 add per word (numpy); overflow to +-inf is a value like any other"""
    with np.errstate(over="ignore"):
        return (acc.astype(np.float32) + wide.astype(np.float32)).astype(np.float32)


def random_acc(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 3.0).numpy()


def block_words(ans_archive):
    """compressed 16-bit words of every block of an ANS archive: the low half of each {sizes, start} descriptor, which
    follow the 32-byte header, the 512-byte pdf table and 128 bytes of lane states per block"""
    hdr = ans_archive[:32].view(np.uint32)
    nb = int(hdr[1])
    off = 32 + 512 + 128 * nb
    bw = ans_archive[off : off + 8 * nb].view(np.uint32).reshape(nb, 2)
    return bw[:, 0] & 0xFFFF


def ans_offset(ft, n):
    """where the ANS archive begins inside a float archive of n words"""
    return 16 + O.float_uncomp_data_size(ft, n)


def float_block_words(ft, archive, n):
    return block_words(archive[ans_offset(ft, n):])


class Case:
    """The elements of one test case: words, their widening, oracle archives, starting accumulators and expected
    sums -- each computed once and shared."""

    def __init__(self, tag, ft, specs):
        """specs: per element (kinds of the whole blocks, words of the partial last block, its kind, seed)"""
        self.tag, self.ft = tag, ft
        self.words = [words(ft, kinds, tail, tail_kind, seed) for kinds, tail, tail_kind, seed in specs]
        self.sizes = [int(w.size) for w in self.words]
        self.kinds = [kinds + (tail_kind if tail else "") for kinds, tail, tail_kind, _ in specs]  # of every block

    @functools.cached_property
    def wide(self):
        return [widen(self.ft, w) for w in self.words]

    @functools.lru_cache(maxsize=None)
    def archives(self, prob_bits):
        return [O.float_compress(self.ft, w, prob_bits) for w in self.words]

    @functools.cached_property
    def start(self):
        return [random_acc(n, zlib.crc32(f"{self.tag}/{self.ft}/{i}".encode())) for i, n in enumerate(self.sizes)]

    @functools.lru_cache(maxsize=None)
    def sums(self, reps=1):
        """start + wide, `reps` times over"""
        out = []
        for s, w in zip(self.start, self.wide):
            for _ in range(reps):
                s = add(s, w)
            out.append(s)
        return out


# ------------------------------------------------------------------------------------------------ 1. staging modes
# the shapes of test_decoder_staging_modes_raw: waves of both kinds and waves that mix them, in 16-block tiles (41, 34 and
# 24 blocks) and 4-block ones, partial last blocks of 777, 4095 and 1 words, and 24 blocks at the staging limit
STAGING_SHAPES = [("ccrrcrrc" * 5, 777), ("ccrcrr", 0), ("cc", 0), ("rr", 0), ("c" * 33, 4095), ("rc", 1), ("b" * 24, 0)]
STAGING_MIXED, STAGING_BOUNDARY = 0, 6  # the two elements the ranged decode test uses
# seeds (per variant) at which the "b" element has blocks on both sides of 1024 words at probBits 9, 10 AND 11 -- at
# 11 only about one block in ten is above; the host test asserts it for the elements used
STAGING_SEEDS = (11, 12)


@functools.lru_cache(maxsize=None)
def staging(ft, variant=0):
    seed = STAGING_SEEDS[variant]
    return Case(f"staging{variant}", ft, [(kinds, tail, "c", 1000 * seed + i) for i, (kinds, tail) in enumerate(STAGING_SHAPES)])


def wave_kinds(counts):
    """{'whole/whole', 'ring/ring', 'mixed', 'boundary'} -> waves of an element with these block word counts.  A wave
    decodes blocks 2k and 2k + 1 (tiles hold an even number of blocks); a last wave may hold one block.  'boundary': a
    wave with a block within 8 words of the limit."""
    out = {"whole/whole": 0, "ring/ring": 0, "mixed": 0, "boundary": 0}
    for k in range(0, len(counts), 2):
        pair = [int(c) for c in counts[k : k + 2]]
        small = [c <= STAGE_WORDS for c in pair]
        out["whole/whole" if all(small) else "mixed" if any(small) else "ring/ring"] += 1
        out["boundary"] += any(abs(c - STAGE_WORDS) <= 8 for c in pair)
    return out


# ---------------------------------------------------------------------------------------- 2. partial last blocks
LASTS = [1, 31, 32, 33, 255, 256, 257, 288, 1023, 1024, 2049, 3585, 3840, 3841, 4064, 4065, 4095]
LEADS = (0, 1, 3, 8)


@functools.lru_cache(maxsize=None)
def tails(ft, lead):
    rng = np.random.default_rng(9100 + lead)
    lasts = LASTS + [int(n) for n in rng.integers(1, BLK, 8)]
    return Case(f"tails{lead}", ft, [("cr"[i % 2] * lead, n, "cr"[i % 2], 20000 + 100 * lead + i) for i, n in enumerate(lasts)])


# ------------------------------------------------------------------------------------------- 3. workgroup orders
ORDER_BATCHES = (8, 13, 64, 67)
ORDER_GEOMETRIES = {4: (5, 8), 16: (17, 32)}  # blocks per tile -> element sizes in blocks: two tiles each


@functools.lru_cache(maxsize=None)
def orders(ft, B, tile_blocks):
    lo, hi = ORDER_GEOMETRIES[tile_blocks]
    rng = np.random.default_rng(300 + 7 * B + tile_blocks)
    specs = []
    for i in range(B):
        nb = int(rng.integers(lo, hi + 1))
        if i == 0:
            nb = hi  # the call's geometry and its two tiles per element
        tail = int(rng.integers(1, BLK)) if i % 2 else 0
        whole = nb - 1 if tail else nb
        # at least half of the blocks "c", at least one "r", in random order: the element's table is built from all of its
        # blocks, and beside too many uniform ones a "c" block would no longer compress to 1024 words
        nc = int(rng.integers((whole + 1) // 2, whole))
        kinds = "".join(rng.permutation(["c"] * nc + ["r"] * (whole - nc)))
        specs.append((kinds, tail, "cr"[i % 2], 30000 + 1000 * B + 10 * i + tile_blocks))
    return Case(f"orders{B}x{tile_blocks}", ft, specs)


def tiles_of(sizes, tile_blocks):
    return [max(1, -(-n // (tile_blocks * BLK))) for n in sizes]


# ------------------------------------------------------------------------------ 4. capacity larger than the element
CAPACITY_SIZES = (1, BLK + 1, 3 * BLK + 5, 17 * BLK)


def _round_up(n, m):
    return -(-n // m) * m


CAPACITY_RULES = {
    "one more word": lambda n: n + 1,
    "a multiple of 8 blocks": lambda n: _round_up(n, 8 * BLK),
    "a multiple of 16 blocks": lambda n: _round_up(n, 16 * BLK),
    "40 blocks": lambda n: 40 * BLK,
}


@functools.lru_cache(maxsize=None)
def capacity(ft):
    return Case("capacity", ft, [("cr" * (n // BLK // 2) + "c" * (n // BLK % 2), n % BLK, "r", 40000 + i)
                                 for i, n in enumerate(CAPACITY_SIZES)])


# --------------------------------------------------------------------------------- 5. accumulators as matrix rows
ROW_WORDS = BLK * 5 + 123
ROW_ORDERS = ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [3], [0, 2, 4], [4, 0, 5, 1])


@functools.lru_cache(maxsize=None)
def rows(ft):
    return Case("rows", ft, [("crrcc"[i % 5 :] + "crrcc"[: i % 5], 123, "cr"[i % 2], 50000 + i) for i in range(6)])


# -------------------------------------------------------------------------------------- 6. malformed descriptors
# name -> (blocks per tile, [left neighbour, the element that gets corrupted, right neighbour], capacity of the middle one)
MALFORMED_BATCHES = {
    "three 16-block tiles": (16, [17 * BLK + 5, 39 * BLK + 100, 33 * BLK], 39 * BLK + 100),
    "two 4-block tiles": (4, [5 * BLK + 7, 6 * BLK + 100, 8 * BLK], 8 * BLK),
}


@functools.lru_cache(maxsize=None)
def malformed(ft, name):
    sizes = MALFORMED_BATCHES[name][1]
    return Case("malformed " + name, ft, [(("ccrcrr" * 7)[: n // BLK], n % BLK, "cr"[i % 2], 60000 + 10 * len(name) + i)
                                          for i, n in enumerate(sizes)])


def corruptions(ft, good, n, tile_blocks):
    """-> [(name, archive)]: the descriptor corruptions of test_decoder_rejects_malformed_ans_archives, each applied
    on its own to a block of the first tile and to a block of the last tile of an element of n words (whose last block
    is partial; the wrong size of the LAST block exists in the last tile only), and a pdf table that no longer sums to
    2^probBits"""
    nb = -(-n // BLK)
    assert n % BLK and nb > tile_blocks
    ans = ans_offset(ft, n)
    bw0 = ans + 32 + 512 + 128 * nb
    u32 = lambda off: int(good[off : off + 4].view(np.uint32)[0])
    first_tile, last_tile = 1, (nb - 1) // tile_blocks * tile_blocks + 1  # odd blocks: the upper half of a wave
    assert last_tile < nb - 1
    out = []
    for where, blk in (("first tile", first_tile), ("last tile", last_tile)):
        d = bw0 + 8 * blk
        out += [
            (f"block {blk} ({where}): uncompressed size", d, (4095 << 16) | (u32(d) & 0xFFFF)),
            (f"block {blk} ({where}): start past the end", d + 4, u32(ans + 12)),
            (f"block {blk} ({where}): start unaligned", d + 4, u32(d + 4) + 3),
        ]
    d = bw0 + 8 * (nb - 1)
    out.append((f"block {nb - 1} (last tile): the last block's size", d, ((n % BLK + 1) << 16) | (u32(d) & 0xFFFF)))
    cases = []
    for name, off, val in out:
        bad = good.copy()
        bad[off : off + 4].view(np.uint32)[0] = val
        cases.append((name, bad))
    bad = good.copy()
    bad[ans + 32 : ans + 34].view(np.uint16)[0] += 1
    cases.append(("pdf table does not sum to 2^probBits", bad))
    return cases


def all_cases(ft):
    """every case of the GPU tests as (case, number of successive adds)"""
    out = [(staging(ft, 0), 3), (staging(ft, 1), 3)]
    out += [(tails(ft, lead), 1) for lead in LEADS]
    out += [(orders(ft, B, tb), 1) for B in ORDER_BATCHES for tb in ORDER_GEOMETRIES]
    out += [(capacity(ft), 1), (rows(ft), 1)]
    out += [(malformed(ft, name), 1) for name in MALFORMED_BATCHES]
    return out
