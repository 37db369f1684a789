"""XOR-delta archives on the GPU (dgpu_ans_delta_encode / dgpu_ans_delta_decode): the archive must be byte for byte the
oracle's raw-byte archive of in ^ base (numpy XOR + oracle.ans_encode), and the decode must restore `in` bit for bit --
into a separate output, in place into a copy of the base, and through the EXISTING raw decoder plus a host XOR."""
import numpy as np
import pytest
import torch

import dietgpu_amd as dg
import oracle as O

pytestmark = pytest.mark.gpu

BLK = 4096
# partial / full / odd block counts, one 8-block encode tile, a 16-block decode tile plus a tail, more than one
# look-back group of encode tiles, and one batch that mixes size classes
BATCHES = [[1], [4095], [4096], [4097], [2 * BLK + 5], [8 * BLK], [16 * BLK + 17], [65 * 8 * BLK], [100, 3 * BLK, 40 * BLK]]
# data: a quarter of the bf16 words moved one ulp / in == base (the one-symbol table) / independent random bytes
# (the last two cases: `in` and `base` 4 and 12 bytes into their allocations, so that they differ modulo 16)
CASES = [(b, k, 10, "torch_ops", (0, 0)) for b in BATCHES for k in ("ulp", "same", "random")] + \
        [(b, "ulp", p, "ctypes", (0, 0)) for b in ([4097], [16 * BLK + 17], BATCHES[-1]) for p in (10, 9, 11)] + \
        [(b, "ulp", 10, "ctypes", (4, 12)) for b in ([16 * BLK + 17], BATCHES[-1])]
_cache = {}
_bytes = lambda t: t.view(torch.uint8).cpu().numpy()


def _pair(kind, n, salt):
    """-> (in, base) as n bytes each; base: bf16 N(0, 0.02) words"""
    key = (kind, n, salt)
    if key not in _cache:
        rng = np.random.default_rng(977 * salt + n)
        words = (n + 1) // 2
        base = ((rng.standard_normal(words) * 0.02).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        new = base + (rng.integers(0, 4, words) == 0).astype(np.uint16) * (kind == "ulp")
        if kind == "random":
            new = rng.integers(0, 1 << 16, words, dtype=np.uint16)
        _cache[key] = (new.view(np.uint8)[:n].copy(), base.view(np.uint8)[:n].copy())
    return _cache[key]


def _want(kind, n, salt, prob_bits):
    """the reference archive, computed once per case"""
    key = ("ref", kind, n, salt, prob_bits)
    if key not in _cache:
        a, b = _pair(kind, n, salt)
        _cache[key] = O.ans_encode(a ^ b, prob_bits)
    return _cache[key]


def _gpu(x, lead=0):
    """the bytes on the GPU, `lead` bytes into their allocation; as bfloat16 where the size and the offset allow"""
    t = torch.zeros(x.size + lead, dtype=torch.uint8, device="cuda:0")[lead:]
    t.copy_(torch.from_numpy(x))
    return t.view(torch.bfloat16) if x.size % 2 == 0 and lead % 2 == 0 else t


def _routed(route, fn, *args, **kw):
    dg.prefer_torch_ops(route == "torch_ops")
    try:
        return fn(*args, **kw)
    finally:
        dg.prefer_torch_ops(True)


@pytest.mark.parametrize("sizes,kind,prob_bits,route,leads", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, (list, tuple)) else str(v))
def test_archive_is_the_oracles_and_every_decoder_restores_the_tensor(sizes, kind, prob_bits, route, leads):
    pairs = [_pair(kind, n, i) for i, n in enumerate(sizes)]
    ins, bases = [_gpu(a, leads[0]) for a, _ in pairs], [_gpu(b, leads[1]) for _, b in pairs]
    comp, csizes = _routed(route, dg.compress_data_delta, ins, bases, prob_bits=prob_bits)
    rows = []
    for i, n in enumerate(sizes):
        want = _want(kind, n, i, prob_bits)
        assert int(csizes[i]) == want.size, (i, n)
        rows.append(comp[i, : want.size])
        assert np.array_equal(rows[i].cpu().numpy(), want), (i, n)
        assert np.array_equal(_bytes(ins[i]), pairs[i][0]) and np.array_equal(_bytes(bases[i]), pairs[i][1])  # inputs untouched
    # separate outputs, then in place into clones of the bases
    outs, inplace = [torch.full_like(b, 7) for b in bases], [b.clone() for b in bases]
    for dst in (outs, None):
        status = torch.full((len(sizes),), 9, dtype=torch.uint8, device="cuda:0")
        dsizes = torch.full((len(sizes),), -9, dtype=torch.int32, device="cuda:0")
        _routed(route, dg.decompress_data_delta, rows, bases if dst else inplace, dst, status, dsizes, prob_bits=prob_bits)
        assert status.tolist() == [1] * len(sizes) and dsizes.tolist() == sizes
    # an ordinary archive: the existing raw decoder, XOR-ed with the base on the host
    plain = [torch.empty(n, dtype=torch.uint8, device="cuda:0") for n in sizes]
    dg.decompress_data(False, rows, plain, prob_bits=prob_bits)
    for i in range(len(sizes)):
        assert np.array_equal(_bytes(outs[i]), pairs[i][0]) and np.array_equal(_bytes(inplace[i]), pairs[i][0]), i
        assert np.array_equal(_bytes(plain[i]) ^ pairs[i][1], pairs[i][0]), i


@pytest.mark.parametrize("fault", ["truncated", "capacity"])
@pytest.mark.parametrize("route", ["torch_ops", "ctypes"])
def test_a_failing_member_keeps_its_base_and_the_others_are_restored(fault, route):
    pairs = [_pair("ulp", n, i) for i, n in enumerate([4097, 16 * BLK + 17, 5001])]
    comp, csizes = dg.compress_data_delta([_gpu(a) for a, _ in pairs], [_gpu(b) for _, b in pairs])
    rows, work = [comp[i, : int(csizes[i])] for i in range(3)], [_gpu(b) for _, b in pairs]
    if fault == "truncated":
        rows[1] = rows[1][: rows[1].numel() - 16]
    else:
        work[1] = _gpu(pairs[1][1][:-1])  # outCapacity one byte short
    before = _bytes(work[1]).copy()
    status = torch.full((3,), 9, dtype=torch.uint8, device="cuda:0")
    _routed(route, dg.decompress_data_delta, rows, work, None, status)  # in place
    assert status.tolist() == [1, 0, 1] and np.array_equal(_bytes(work[1]), before)
    assert np.array_equal(_bytes(work[0]), pairs[0][0]) and np.array_equal(_bytes(work[2]), pairs[2][0])


def test_nothing_outside_the_outputs_is_written():
    sizes, gap = [4097, 2 * BLK + 5, 16 * BLK + 17, 31], 3
    pairs = [_pair("ulp", n, i) for i, n in enumerate(sizes)]
    bases = [_gpu(b) for _, b in pairs]
    comp, csizes = dg.compress_data_delta([_gpu(a) for a, _ in pairs], bases)
    flat = torch.full((sum(sizes) + gap * (len(sizes) + 1),), 0xA5, dtype=torch.uint8, device="cuda:0")
    at = np.cumsum([gap] + [n + gap for n in sizes[:-1]])
    outs = [flat[a : a + n] for a, n in zip(at.tolist(), sizes)]
    dg.decompress_data_delta([comp[i, : int(csizes[i])] for i in range(len(sizes))], bases, outs)
    want = np.full(flat.numel(), 0xA5, dtype=np.uint8)
    for a, n, (new, _) in zip(at.tolist(), sizes, pairs):
        want[a : a + n] = new
    assert np.array_equal(flat.cpu().numpy(), want)
