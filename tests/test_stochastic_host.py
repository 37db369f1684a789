"""Stochastic cast-compress without a GPU (dgpu_float_stochastic_compress): the entry point is exported and bound, its
declaration has no temp-memory parameters, every invalid argument is refused with DGPU_ERR_INVALID_ARGUMENT and a text
before anything is enqueued (no call here reaches a device), the empty batch returns 0, the argument checks of
ops.compress_data_stochastic raise RuntimeError, the torch restatement of the rounding gives the reference's words, a
reference archive decodes to the reference's words, and the rounding is unbiased within 5 sigma."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import oracle as O
import sr_ref as S
import stochastic_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dgpu_float_stochastic_compress"
_TORCH = {S.BFLOAT16: torch.bfloat16, S.FLOAT16: torch.float16}


def _declaration():
    text = open(os.path.join(ROOT, "include", "dietgpu_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    (params,) = re.findall(r"\b%s\s*\(([^;{]*?)\)\s*;" % NAME, text, flags=re.S)
    return params


def test_the_declaration_has_no_temp_memory_parameters():
    params = _declaration()
    for name in ("temp_dev", "tempBytes", "tempUsed"):
        assert not re.search(r"\b%s\b" % name, params), name
    names = [p.split()[-1].lstrip("*") for p in params.split(",")]
    assert names == ["floatType", "probBits", "numInBatch", "in", "inSize", "seed", "seed_dev", "firstMember", "out", "outSize_dev", "stream"]
    header = open(os.path.join(ROOT, "include", "dietgpu_amd.h")).read()
    doc = header[header.index("---- stochastic cast-compress"): header.index("int " + NAME)]
    assert "no temp-memory parameters" in doc and "dgpu_float_decode_update" in doc
    # the constants of the rounding are stated once, under decode-update
    assert "0x7feb352d" not in doc and "0x85EBCA6B" not in doc
    assert "#define DGPU_ABI_VERSION 8u" in header and NAME in header[: header.index("#define DGPU_ABI_VERSION")]
    for claimed in ("float_compress", "float_decompress", "encode_batch", "decode_batch"):  # (tests/test_cabi_argument_errors.py's table)
        assert claimed not in NAME


def test_entry_point_is_exported_and_bound():
    import dietgpu_amd
    from dietgpu_amd import distributed

    raw = ctypes.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    assert NAME in dietgpu_amd.EXPORTED_SYMBOLS and hasattr(raw, NAME)
    assert len(getattr(L, NAME).argtypes) == 11 and getattr(L, NAME).restype is ctypes.c_int
    assert L.dgpu_abi_version() == 8
    assert callable(dietgpu_amd.compress_data_stochastic)
    assert list(inspect.signature(dietgpu_amd.compress_data_stochastic).parameters) == [
        "ts_in", "dtype", "seed", "first_member", "out_compressed", "out_compressed_sizes", "prob_bits"]
    assert list(inspect.signature(distributed.GpuFloatCodec.compress_cast_stochastic).parameters) == [
        "self", "tensors", "dtype", "seed", "first_member"]
    assert "wire_seed" in inspect.signature(distributed.compressed_all_reduce).parameters
    assert "wire_seed" in inspect.signature(distributed.compressed_reduce_scatter).parameters
    assert "same on every rank" in distributed.compressed_reduce_scatter.__doc__.lower()


def test_argument_errors_of_the_c_abi_need_no_device():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    f = getattr(L, NAME)
    one = (ctypes.c_uint32 * 1)(16)
    src = (ctypes.c_void_p * 1)(4096)  # "device" addresses that are never followed: every call below fails before a launch
    dst = (ctypes.c_void_p * 1)(8192)
    dummy = ctypes.c_void_p(4096)

    def fails(message, ft=2, P=10, n=1, ins=src, sizes=one, seed=1, seed_dev=None, first=0, outs=dst):
        assert f(ft, P, n, ins, sizes, seed, seed_dev, first, outs, None, None) == 1
        text = L.dgpu_last_error().decode()
        assert message in text and text, text

    fails("floatType", ft=3)  # DGPU_FLOAT32 is rejected
    fails("floatType", ft=0)
    fails("floatType", ft=4)
    fails("probBits must be 9, 10 or 11", P=8)
    fails("probBits must be 9, 10 or 11", P=12)
    fails("numInBatch must be <= 65535", n=65536)
    fails("seed_dev must be 8-byte aligned", seed_dev=ctypes.c_void_p(4100))
    fails("seed_dev must be 8-byte aligned", seed_dev=ctypes.c_void_p(4097), seed=0)
    for missing in ("ins", "sizes", "outs"):
        fails("null array", **{missing: None})
        fails("null array", seed_dev=dummy, **{missing: None})
    fails("4-byte aligned", ins=(ctypes.c_void_p * 1)(4096 + 2))
    fails("16-byte aligned", outs=(ctypes.c_void_p * 1)(8192 + 8))
    fails("larger than 1717538816", sizes=(ctypes.c_uint32 * 1)(1717538816 + 1))
    two = (ctypes.c_uint32 * 2)(16, 0xFFFFFFFF)
    fails("larger than 1717538816", n=2, ins=(ctypes.c_void_p * 2)(4096, 4096 + 64), sizes=two, outs=(ctypes.c_void_p * 2)(8192, 16384))
    # an empty batch is fine
    assert f(2, 10, 0, None, None, 1, None, 0, None, None, None) == 0
    assert f(1, 9, 0, None, None, 2**64 - 1, dummy, 2**32 - 1, None, None, None) == 0


@pytest.mark.parametrize("torch_ops", [True, False])
def test_rejects_bad_arguments_without_a_gpu(torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        x = torch.zeros(4096, dtype=torch.float32)  # CPU tensors
        with pytest.raises(RuntimeError, match="on the GPU"):
            dg.compress_data_stochastic([x], torch.bfloat16, 1)
        with pytest.raises(RuntimeError):
            dg.compress_data_stochastic([], torch.bfloat16, 1)
        for bad in (torch.float32, torch.uint8, None):
            with pytest.raises(RuntimeError, match="float16 or bfloat16"):
                dg.compress_data_stochastic([x], bad, 1)
        with pytest.raises(RuntimeError, match="must be float32"):
            dg.compress_data_stochastic([x.to(torch.bfloat16)], torch.bfloat16, 1)
        for bad in (-1, 2**64, 1.5, True, None, "seed"):
            with pytest.raises(RuntimeError, match="seed must be"):
                dg.compress_data_stochastic([x], torch.bfloat16, bad)
        for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.float32)):
            with pytest.raises(RuntimeError, match="1-element int64"):
                dg.compress_data_stochastic([x], torch.float16, bad)
        with pytest.raises(RuntimeError, match="on the tensors' GPU"):  # a CPU seed tensor
            dg.compress_data_stochastic([x], torch.float16, torch.zeros(1, dtype=torch.int64))
        for bad in (-1, 2**32, 0.5, True):
            with pytest.raises(RuntimeError, match="first_member"):
                dg.compress_data_stochastic([x], torch.bfloat16, 1, first_member=bad)
    finally:
        dg.prefer_torch_ops(True)


def _bits(n, seed):
    """N(0, 1) * 2^k and random bit patterns by halves: NaNs, infinities, denormals among them"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32).view(np.uint32)
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return np.where(np.arange(n) % 2 == 0, a, b).astype(np.uint32)


@pytest.mark.parametrize("ft", [S.BFLOAT16, S.FLOAT16])
@pytest.mark.parametrize("n", [1, 7, 4097])
def test_the_torch_restatement_gives_the_reference_words(ft, n):
    from dietgpu_amd import rounding

    for seed, member in ((0, 0), (0x0123456789ABCDEF, 3), (2**64 - 1, 65534)):
        bits = _bits(n, n + member)
        value = torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32)
        out = torch.empty((n,), dtype=_TORCH[ft])
        assert rounding.stochastic_round_(out, value, seed, member) is out
        got = out.view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got, SR.words(bits, ft, seed, member)), (ft, n, seed, member)
        # a tensor seed holds the same 64 bits
        held = torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.int64)
        out2 = torch.empty((n,), dtype=_TORCH[ft])
        rounding.stochastic_round_(out2, value, held, member)
        assert torch.equal(out2.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("ft", [S.BFLOAT16, S.FLOAT16])
def test_a_reference_archive_decodes_to_the_reference_words(ft):
    for n, prob_bits in ((1, 10), (4097, 9), (2 * 4096 + 5, 11)):
        bits = _bits(n, n)
        arch, words = SR.archive(bits, ft, 12345678901234567, 7, prob_bits)
        rc, got, size = O.float_decompress(ft, arch, prob_bits)
        assert rc == 0 and size == n and np.array_equal(got, words)
        # a representable value never moves; the member and the seed matter
        exact = (words.astype(np.uint32) << 16) if ft == S.BFLOAT16 else None
        if exact is not None:
            assert np.array_equal(SR.words(exact, ft, 99, 1), words)
    big = _bits(4096, 5)
    assert not np.array_equal(SR.words(big, ft, 1, 0), SR.words(big, ft, 2, 0))
    assert not np.array_equal(SR.words(big, ft, 1, 0), SR.words(big, ft, 1, 1))


#   (float type, x, the word toward zero, probability of the next word away from zero)
FREQUENCY = [(S.BFLOAT16, 0x3F802000, 0x3F80, 1 / 8), (S.FLOAT16, 0x3F800400, 0x3C00, 1 / 8), (S.BFLOAT16, 0x3F80E000, 0x3F80, 7 / 8),
             (S.FLOAT16, 0x33A00000, 0x0001, 1 / 4)]
STREAMS = [(0, 0), (1, 0), (12345678901234567, 3), (2**64 - 1, 65534), (7, 257)]


@pytest.mark.parametrize("seed,member", STREAMS)
@pytest.mark.parametrize("ft,x,low,p", FREQUENCY)
def test_the_rounding_is_unbiased_within_five_sigma(ft, x, low, p, seed, member):
    """65536 equal words of one member: only the two neighbours occur, and the number rounded away from zero lies within
    5 sqrt(N p (1 - p)) of N p"""
    N = 65536
    words = SR.words(np.full(N, x, dtype=np.uint32), ft, seed, member)
    away = int((words == low + 1).sum())
    assert away + int((words == low).sum()) == N, "a word that is neither neighbour"
    sigma = math.sqrt(N * p * (1 - p))
    print(f"ft={ft} x={x:#x} seed={seed} member={member}: {away} of {N} away, expected {N * p:.0f}, {(away - N * p) / sigma:+.2f} sigma")
    assert abs(away - N * p) <= 5 * sigma
