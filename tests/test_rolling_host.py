"""Rolling-table compress, the parts that need no GPU: the entry point is exported and bound, its argument checks (code 1
and the literal message, before anything touches a device) and those of the Python layer, and the pins of the reference
helper itself (tests/rolling_ref.py): composed with the data's own histogram it IS the oracle's float archive, smoothed
tables give every symbol a probability, and archives of stale or hostile tables decode back bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
import rolling_ref as R

A = 0x10000  # a fake device address, aligned to everything
TOO_LARGE = 1717538816 + 1
NAME = "dgpu_float_rolling_compress"


def test_rolling_entry_point_is_exported_and_bound():
    import dietgpu_amd

    raw = C.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    assert NAME in dietgpu_amd.EXPORTED_SYMBOLS and hasattr(raw, NAME)
    assert getattr(L, NAME).argtypes is not None and getattr(L, NAME).restype is C.c_int
    assert L.dgpu_abi_version() == 8  # an added entry point does not move the version
    assert callable(dietgpu_amd.compress_data_rolling)
    from dietgpu_amd import distributed

    assert distributed.GpuFloatCodec(rolling=True).rolling and not distributed.GpuFloatCodec().rolling


def _call(n=1, floatType=2, cast=0, probBits=10, inp=None, sizes=None, out=None, cin=A, cout=A):
    import dietgpu_amd

    L = dietgpu_amd.lib()
    used = C.c_size_t(77)
    inp = (C.c_void_p * max(n, 1))(*(inp if inp is not None else [A] * n))
    out = (C.c_void_p * max(n, 1))(*(out if out is not None else [A] * n))
    sizes = (C.c_uint32 * max(n, 1))(*(sizes if sizes is not None else [4096] * n))
    rc = getattr(L, NAME)(None, 0, C.byref(used), floatType, cast, probBits, n, inp, sizes, cin, cout, out, None, None)
    return rc, L.dgpu_last_error().decode(), used.value


_MSG_FT = "rolling compress: floatType of the archive must be float16 or bfloat16 (float32 archives: dgpu_float_compress)"
_MSG_COUNTS = "rolling compress: counts must be 4-byte aligned"
_MSG_SIZE = ("tensor larger than 1717538816 words: the maximum compressed size of its exponent plane exceeds INT32_MAX "
             "(GpuANSEncode.cu:22)")


@pytest.mark.parametrize("over,message", [
    (dict(floatType=0), _MSG_FT),
    (dict(floatType=3), _MSG_FT),
    (dict(floatType=3, cin=None, cout=None), _MSG_FT),
    (dict(floatType=4), _MSG_FT),
    (dict(cast=2), "rolling compress: sourceFloat32 must be 0 or 1"),
    (dict(cin=A + 2), _MSG_COUNTS),
    (dict(cout=A + 1), _MSG_COUNTS),
    (dict(cin=None, cout=A + 2), _MSG_COUNTS),
    (dict(n=2, cin=A, cout=A + 1024), "rolling compress: countsIn_dev and countsOut_dev must be the same buffer or not overlap"),
    (dict(n=2, inp=[A, A + 1]), "float input must be float-word aligned"),
    (dict(n=2, cast=1, inp=[A, A + 2]), "float32 input must be 4-byte aligned"),
    (dict(n=2, out=[A, A + 8]), "compressed output must be 16-byte aligned"),
    (dict(probBits=8), "probBits must be 9, 10 or 11"),
    (dict(probBits=12), "probBits must be 9, 10 or 11"),
    (dict(probBits=12, cin=None, cout=None), "probBits must be 9, 10 or 11"),
    (dict(n=65536), "numInBatch must be <= 65535"),
    (dict(sizes=[TOO_LARGE]), _MSG_SIZE),
    (dict(sizes=[TOO_LARGE], cin=None), _MSG_SIZE),
])
def test_one_fault_gives_this_code_and_text(over, message):
    rc, text, _ = _call(**over)
    assert (rc, text) == (1, message)  # DGPU_ERR_INVALID_ARGUMENT


def test_an_empty_batch_ends_after_the_checks():
    for ft in (1, 2):
        for cast in (0, 1):
            for cin, cout in ((A, A), (None, A), (A, None), (None, None), (A, A + 4096)):
                rc, _, used = _call(n=0, floatType=ft, cast=cast, cin=cin, cout=cout)
                assert rc == 0 and used == 0


@pytest.mark.parametrize("torch_ops", [True, False])
def test_ops_reject_bad_arguments_without_a_gpu(torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        x = torch.zeros(4096, dtype=torch.bfloat16)  # a CPU tensor
        with pytest.raises(RuntimeError):
            dg.compress_data_rolling([x], None, None)
        with pytest.raises(RuntimeError):
            dg.compress_data_rolling([], None, None)
        with pytest.raises(RuntimeError):  # float32 tensors need the archives' dtype
            dg.compress_data_rolling([x.float()], None, None)
        for bad in (torch.float32, torch.float64, torch.int16):
            with pytest.raises(RuntimeError):
                dg.compress_data_rolling([x.float()], None, None, dtype=bad)
        with pytest.raises(RuntimeError):  # counts on the CPU
            dg.compress_data_rolling([x], torch.zeros(1, 256, dtype=torch.int32), None)
    finally:
        dg.prefer_torch_ops(True)


# ---------------------------------------------------------------------------------------------- the helper's own pins
def _words(rng, ft, n, scale=1.0):
    f = (rng.standard_normal(n) * scale).astype(np.float32)
    if ft == R.BFLOAT16:
        return (f.view(np.uint32) >> 16).astype(np.uint16)
    return f.astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("ft", [R.FLOAT16, R.BFLOAT16])
@pytest.mark.parametrize("prob_bits", [9, 10, 11])
def test_composition_with_the_datas_own_histogram_is_the_oracles_float_archive(ft, prob_bits):
    rng = np.random.default_rng(ft * 100 + prob_bits)
    for n in (1, 31, 4095, 4096, 4097, 2 * 4096 + 33, 69732):
        w = _words(rng, ft, n)
        want = O.float_compress(ft, w, prob_bits)
        got = R.expected_archive(ft, w, prob_bits, R.exponent_hist(ft, w))
        assert got.size == want.size and (got == want).all(), (n, got.size, want.size)
        assert R.sizes_blockwise(ft, w, prob_bits, R.exponent_hist(ft, w)) == want.size
        assert R.exponent_hist(ft, w).sum() == n and (R.exponent_bytes(ft, w) == O.float_split(ft, w)[0]).all()


@pytest.mark.parametrize("prob_bits", [9, 10, 11])
def test_smoothed_tables_give_every_symbol_a_probability(prob_bits):
    rng = np.random.default_rng(prob_bits)
    n = 5 * 4096 + 7
    for counts in (np.zeros(256, np.uint32), np.full(256, 0xFFFFFFFF, np.uint32), R.exponent_hist(R.BFLOAT16, np.zeros(n, np.uint16)),
                   rng.integers(0, 1 << 32, 256, dtype=np.uint64).astype(np.uint32), R.exponent_hist(R.BFLOAT16, _words(rng, R.BFLOAT16, n))):
        c = R.smooth(counts, n)
        assert c.min() >= 1 and c.max() <= n
        table = O.normalize(c, n, prob_bits)
        assert table[:, 0].min() >= 1 and int(table[:, 0].sum()) == 1 << prob_bits
    assert (R.smooth(np.array([0, 1, 5, 9], np.uint32), 5) == [1, 1, 5, 5]).all()


@pytest.mark.parametrize("ft", [R.FLOAT16, R.BFLOAT16])
@pytest.mark.parametrize("prob_bits", [9, 10, 11])
def test_stale_and_hostile_tables_round_trip(ft, prob_bits):
    rng = np.random.default_rng(7 * ft + prob_bits)
    n = 9 * 4096 + 7
    x1 = _words(rng, ft, n, 3.0)
    random_bits = rng.integers(0, 1 << 16, n, dtype=np.uint16)
    stale = R.exponent_hist(ft, _words(rng, ft, n))
    hostile = R.exponent_hist(ft, np.zeros(n, np.uint16))
    for w, raw in ((x1, stale), (random_bits, hostile), (random_bits, np.zeros(256, np.uint32)),
                   (random_bits, np.full(256, 0xFFFFFFFF, np.uint32))):
        counts = R.smooth(raw, n)
        arch = R.expected_archive(ft, w, prob_bits, counts)
        assert arch.size == R.sizes_blockwise(ft, w, prob_bits, counts)
        rc, out, size = O.float_decompress(ft, arch, prob_bits)
        assert rc == 0 and size == n and (out == w).all()
    # a table that covers nothing costs about prob_bits bits per symbol: far above the data's own
    own = R.sizes_blockwise(ft, random_bits, prob_bits, R.exponent_hist(ft, random_bits))
    assert R.sizes_blockwise(ft, random_bits, prob_bits, R.smooth(hostile, n)) > own
