"""The premises of tests/accum_cases.py, checked with the CPU oracle (no GPU): what the accumulate and ranged-decode
path tests assume about their inputs -- which staging mode a block takes, that every word is finite, that no expected
sum is NaN -- is asserted here from the very archives those tests decode."""
import numpy as np
import pytest

import accum_cases as C
import oracle as O


@pytest.mark.parametrize("ft", C.FTS)
def test_builders_set_the_compressed_byte(ft):
    rng = np.random.default_rng(1)
    for kind, allowed in (("c", C.C_BYTES[ft]), ("b", C.B_BYTES)):
        w = C.block(ft, kind, 5000, rng, rng)
        comp, _ = O.float_split(ft, w)
        assert set(np.unique(comp).tolist()) == set(int(v) for v in allowed)
        assert C.finite(ft, w).all()
    w = C.block(ft, "r", 1 << 16, rng, rng)
    assert C.finite(ft, w).all()
    assert np.unique(O.float_split(ft, w)[0]).size >= 248  # (an all-ones exponent folds into its neighbour)
    # the exponent mask is the format's: the widened values agree
    for kind in "crb":
        assert np.isfinite(C.widen(ft, C.block(ft, kind, 5000, rng, rng))).all()
    # the same "b" bytes in every float type
    assert np.array_equal(O.float_split(ft, C.words(ft, "bb", 5, "b", seed=3))[0],
                          O.float_split(O.BFLOAT16, C.words(O.BFLOAT16, "bb", 5, "b", seed=3))[0])


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("prob_bits", C.PROB_BITS)
@pytest.mark.parametrize("ft", C.FTS)
def test_staging_elements_take_the_modes_they_are_named_for(ft, prob_bits, variant):
    case = C.staging(ft, variant)
    seen = {}
    for i, (w, kinds, arch) in enumerate(zip(case.words, case.kinds, case.archives(prob_bits))):
        counts = C.float_block_words(ft, arch, w.size)
        assert counts.size == len(kinds) == -(-w.size // C.BLK)
        full = w.size // C.BLK
        for k, c in zip(kinds[:full], counts[:full]):
            if k == "c":
                assert c <= C.STAGE_WORDS, (i, int(c))
            elif k == "r":
                assert c > C.STAGE_WORDS, (i, int(c))
        if set(kinds) == {"b"}:
            assert (counts <= C.STAGE_WORDS).any() and (counts > C.STAGE_WORDS).any(), counts.tolist()
        seen[i] = C.wave_kinds(counts)
        print(f"ft={ft} probBits={prob_bits} variant={variant} element {i} ({w.size} words): words per block "
              f"{int(counts.min())}..{int(counts.max())}, waves {seen[i]}")
    # what the batch is for: waves of every kind, in 16-block and in 4-block tiles
    total = {k: sum(s[k] for s in seen.values()) for k in seen[0]}
    assert all(total.values()), total
    assert seen[0]["whole/whole"] and seen[0]["ring/ring"] and seen[0]["mixed"]
    assert seen[1]["whole/whole"] and seen[1]["ring/ring"] and seen[1]["mixed"]
    assert seen[6]["boundary"] == 12


@pytest.mark.parametrize("ft", C.FTS)
def test_whole_blocks_of_every_case_take_the_mode_of_their_kind(ft):
    # "c" <= 1024 < "r" in every element of every case at probBits 10, the one the tests below the staging test use
    for case, _ in C.all_cases(ft):
        modes = set()
        for w, kinds, arch in zip(case.words, case.kinds, case.archives(10)):
            full = w.size // C.BLK
            counts = C.float_block_words(ft, arch, w.size)
            assert counts.size == len(kinds)
            for k, c in zip(kinds[:full], counts[:full]):
                assert k == "b" or (c <= C.STAGE_WORDS) == (k == "c"), (case.tag, w.size, k, int(c))
                modes.add(bool(c <= C.STAGE_WORDS))
        assert modes == ({False, True} if any(n >= C.BLK for n in case.sizes) else set()), case.tag  # both staging modes
    # the batches of the workgroup-order test: two tiles per element, a rectangle the policy does not replace by a list
    for B in C.ORDER_BATCHES:
        for tb in C.ORDER_GEOMETRIES:
            tiles = C.tiles_of(C.orders(ft, B, tb).sizes, tb)
            assert min(tiles) == max(tiles) == 2 and 5 * sum(tiles) > 4 * B * max(tiles)


@pytest.mark.parametrize("ft", C.FTS)
def test_no_expected_sum_is_nan(ft):
    for case, reps in C.all_cases(ft):
        for w, wide, start in zip(case.words, case.wide, case.start):
            assert C.finite(ft, w).all() and np.isfinite(wide).all() and np.isfinite(start).all(), case.tag
            assert wide.size == start.size == w.size
        for r in range(1, reps + 1):
            assert not any(np.isnan(s).any() for s in case.sums(r)), (case.tag, r)


@pytest.mark.parametrize("ft", C.FTS)
def test_the_oracle_round_trips_the_cases_and_corruptions_touch_one_field(ft):
    case = C.staging(ft, 0)
    for w, arch in zip(case.words, case.archives(10)):
        rc, out, n = O.float_decompress(ft, arch, 10)
        assert rc == 0 and n == w.size and np.array_equal(out, w)
    for name, (tile_blocks, sizes, _) in C.MALFORMED_BATCHES.items():
        good = C.malformed(ft, name).archives(10)[1]
        bads = C.corruptions(ft, good, sizes[1], tile_blocks)
        assert len(bads) == 8
        for what, bad in bads:
            diff = np.nonzero(bad != good)[0]
            assert 1 <= diff.size <= 4 and diff.max() - diff.min() < 4, what
