"""The vocabulary of the call-state tests (tests/state_cases.py) without a GPU: it names every C-ABI call that takes temp
memory, and every expected value builds from the host references -- so the GPU test cannot drift from them."""
import os
import re

import numpy as np
import pytest

import oracle as O
import state_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def functions_with_temp_memory():
    text = open(os.path.join(ROOT, "include", "dietgpu_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(name for name, params in re.findall(r"\b(dgpu_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S) if re.search(r"\btemp_dev\b", params))


def test_every_call_with_temp_memory_is_in_the_vocabulary_or_allowed_with_a_reason():
    declared = functions_with_temp_memory()
    assert len(declared) >= 30 and "dgpu_float_reduce_compress_norm" in declared and "dgpu_ans_get_compressed_info" in declared
    covered = {c for item in S.ITEMS + S.FAILURES for c in item.calls}
    assert covered <= set(declared), sorted(covered - set(declared))
    for name in declared:
        places = [name in covered, name in S.ALLOWED, name in S.NO_TEMP]
        assert sum(places) == 1, f"{name}: in the vocabulary, the allow-list or the no-temp list exactly once, not {places}"
    assert set(S.ALLOWED) | set(S.NO_TEMP) <= set(declared)
    assert all(len(reason) > 10 for reason in S.ALLOWED.values())
    # the forms allowed to stay out because they use no temp memory say so themselves
    header = open(os.path.join(ROOT, "include", "dietgpu_amd.h")).read()
    for name in S.NO_TEMP:
        doc = header[: header.index(f"int {name}(")]
        # (the mixed and scaled decode-reduce take their temp-memory contract from dgpu_float_decode_reduce's text)
        assert "No temp memory is used" in doc[doc.rindex("/* ----"):] or name.startswith("dgpu_float_decode_reduce_"), name


def test_the_cases_have_the_geometry_their_names_promise():
    tiles = lambda n: -(-(-(-n // S.BLK)) // 8)
    sizes = S.CASES["rect"][0]
    assert [tiles(n) for n in sizes] == [3, 3, 3]
    sizes = S.CASES["ragged"][0]
    assert sum(tiles(n) for n in sizes) == 10 and len(sizes) * max(tiles(n) for n in sizes) == 30
    assert sum(tiles(n) for n in sizes) * 5 <= 30 * 4  # listed by policy: at least a fifth of the rectangle does not exist
    sizes = S.CASES["classes"][0]
    assert any(n <= S.BLK for n in sizes) and any(n > 4 * S.BLK for n in sizes)
    assert all(n <= S.BLK for n in S.CASES["pairs"][0]) and 0 in S.CASES["pairs"][0]
    assert all(2 * S.BLK < n <= 4 * S.BLK for n in S.CASES["small-hw"][0])
    assert tiles(S.CASES["deep"][0][0]) == 65  # more than the 64 tiles of one look-back group
    assert S.CASES["large"][0][0] * 2 > 256 * 64 * 1024  # more than 256 histogram workgroups of 64 KiB
    for case, (sizes, noise, _) in S.CASES.items():
        assert all(i < len(sizes) for i in noise), case


def test_every_family_and_every_case_is_in_the_vocabulary():
    names = [i.name for i in S.ITEMS]
    for case in S.CASES:
        assert any(n.endswith("/" + case) for n in names), case
    for tag in ("staging", "tails", "orders67x4"):
        assert any(n.endswith("/" + tag) for n in names), tag
    for family in ("ans-encode-pointer", "ans-encode-stride", "float-compress-bfloat16", "float-compress-float16", "float-compress-float32",
                   "float-compress-capped", "cast-compress", "feedback-compress-fresh", "feedback-compress-in-place", "rolling-compress-counts-out",
                   "rolling-compress-counts-in", "rolling-compress-counts-both", "reduce-compress-plain", "reduce-compress-mixed",
                   "reduce-compress-scaled", "reduce-compress-norm", "decode-reduce-norm", "ans-decode-checksum", "float-decode-checksum"):
        assert any(n.startswith(family) for n in names), family
    assert len(S.FAILURES) == 6 and all(f.failure for f in S.FAILURES) and not any(i.failure for i in S.ITEMS)
    # deep and large: plain float compress and cast-compress only
    for case in ("deep", "large"):
        assert sorted(n.split("-")[0] for n in names if n.endswith("/" + case)) == ["cast", "float"]


@pytest.mark.parametrize("item", S.ITEMS + S.FAILURES, ids=lambda i: i.name)
def test_expected_builds_without_a_gpu(item):
    want = item.expected()
    assert item.expected() is want  # computed once
    for a in want.get("archives", []):
        assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.size >= 16
    for arrays in want.get("arrays", {}).values():
        assert all(isinstance(a, np.ndarray) for a in arrays)
    assert item.query() > 0


def test_the_references_decode_to_the_inputs():
    """the expected archives of a plain, a cast and a rolling item are archives of the case's words"""
    for name, words in (("float-compress-bfloat16/pairs", S.case_words("pairs", O.BFLOAT16)),
                        ("rolling-compress-counts-in-bfloat16/pairs", S.case_words("pairs", O.BFLOAT16))):
        for a, w in zip(S.BY_NAME[name].expected()["archives"], words):
            rc, got, n = O.float_decompress(O.BFLOAT16, a, S.PROB_BITS)
            assert rc == 0 and n == w.size and (got == w).all(), name
    # the clipped rolling archive is longer than the maximum by 16 .. 4096 bytes
    clipped = S.BY_NAME["FAIL rolling compress clipped at the maximum"].expected()
    assert 16 <= clipped["archives"][0].size - clipped["cap"] <= 4096
