"""FP8 archives on the GPU (dgpu_fp8_cast_compress / dgpu_fp8_decode_accumulate), bit for bit against torch's CPU cast:
the archive must be the oracle's raw-byte archive of (x * s).to(float8), the EXISTING raw decoder must return those bytes,
and the accumulating decode must leave bytes.view(float8).float() * s [+ acc] -- a separate multiply and add."""
import numpy as np
import pytest
import torch

import dietgpu_amd as dg
import oracle as O

pytestmark = pytest.mark.gpu

BLK = 4096
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
# partial / full / odd block counts, one 8-block encode tile, a 16-block decode tile plus a tail, more than one
# look-back group of encode tiles, and one batch that mixes size classes
BATCHES = [[1], [4095], [4096], [4097], [2 * BLK + 5], [8 * BLK], [16 * BLK + 17], [65 * 8 * BLK], [100, 3 * BLK, 40 * BLK]]
MODES = ("number", "tensor", "per_member")  # the factor: a Python number, a 1-element device tensor, one per member
# (the last cases: the float32 input 4 and 12 bytes into its allocation)
CASES = [(b, k, dt, 10, "torch_ops", MODES[(i + j) % 3], 0) for i, b in enumerate(BATCHES) for j, k in enumerate(("grad", "edges", "same")) for dt in (E4, E5)] + \
        [(b, "grad", dt, p, "ctypes", "tensor", 0) for b in ([4097], [16 * BLK + 17], BATCHES[-1]) for p in (10, 9, 11) for dt in (E4, E5)] + \
        [(BATCHES[-1], "edges", dt, 10, "ctypes", "per_member", lead) for dt, lead in ((E4, 4), (E5, 12))]
_cache = {}
_u32 = lambda t: t.cpu().contiguous().view(torch.int32).numpy()


def _edges(dtype):
    """every FP8 value, the midpoints between neighbours and one float32 ulp either side, the overflow ties, infinities,
    NaNs, float32 denormals and zeros, both signs -- from torch's own table of the type"""
    vals = torch.arange(256, dtype=torch.uint8).view(dtype).float()
    fin = np.sort(vals[torch.isfinite(vals)].numpy())
    mid = ((fin[:-1].astype(np.float64) + fin[1:]) / 2).astype(np.float32)
    top = np.float32(fin[-1] + (fin[-1] - fin[-2]) / 2)  # the overflow tie: e4m3fn 464, e5m2 61440
    pos = np.array([top, np.nextafter(top, np.float32(0)), np.nextafter(top, np.float32(np.inf)), 2 * top, np.inf, np.nan, 0.0, 1e-45, 1e-39], np.float32)
    mids = np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))])
    return np.concatenate([vals.numpy(), mids, pos, -pos])


def _case(kind, dtype, n, salt, s):
    """-> (x float32 [n], the FP8 bytes of x * s by the CPU cast)"""
    key = (kind, dtype, n, salt, s)
    if key not in _cache:
        rng = np.random.default_rng(977 * salt + n)
        x = (rng.standard_normal(n) * 0.02).astype(np.float32)
        if kind == "edges":
            x = np.resize(_edges(dtype) / np.float32(s), n)
        if kind == "same":
            x = np.full(n, 0.0123, np.float32)
        _cache[key] = (x, (torch.from_numpy(x) * s).to(dtype).view(torch.uint8).numpy())
    return _cache[key]


def _want(key, q, prob_bits):
    if ("ref", key, prob_bits) not in _cache:
        _cache[("ref", key, prob_bits)] = O.ans_encode(q, prob_bits)
    return _cache[("ref", key, prob_bits)]


def _gpu(x, lead=0):
    t = torch.zeros(x.size + lead // 4, dtype=torch.float32, device="cuda:0")[lead // 4:]
    return t.copy_(torch.from_numpy(x))


def _factor(mode, s):
    return s[0] if mode == "number" else torch.tensor(s if mode == "per_member" else s[:1], dtype=torch.float32, device="cuda:0")


@pytest.mark.parametrize("sizes,kind,dtype,prob_bits,route,mode,lead", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v).replace("torch.float8_", ""))
def test_archive_is_the_oracles_and_the_decode_is_the_cpu_composition(sizes, kind, dtype, prob_bits, route, mode, lead):
    s0 = 0.5 if kind == "edges" else 64.0
    s = [s0 * 2.0 ** i if mode == "per_member" else s0 for i in range(len(sizes))]
    data = [_case(kind, dtype, n, i, s[i]) for i, n in enumerate(sizes)]
    ins = [_gpu(x, lead) for x, _ in data]
    dg.prefer_torch_ops(route == "torch_ops")
    try:
        comp, csizes, _ = dg.compress_data_cast(ins, dtype, prob_bits=prob_bits, scale=_factor(mode, s))
        rows = []
        for i, n in enumerate(sizes):
            want = _want((kind, dtype, n, i, s[i]), data[i][1], prob_bits)
            assert int(csizes[i]) == want.size, (i, n)
            rows.append(comp[i, : want.size])
            assert np.array_equal(rows[i].cpu().numpy(), want), (i, n)
            assert np.array_equal(_u32(ins[i]), data[i][0].view(np.int32))  # inputs untouched
        plain = [torch.empty(n, dtype=torch.uint8, device="cuda:0") for n in sizes]
        dg.decompress_data(False, rows, plain, prob_bits=prob_bits)  # an ordinary archive: the existing raw decoder
        inv = [1.0 / v for v in s]
        for accumulate in (False, True):
            start = [torch.from_numpy(np.random.default_rng(n).standard_normal(n).astype(np.float32)) for n in sizes]
            accs = [a.to("cuda:0") for a in start]
            status = torch.full((len(sizes),), 9, dtype=torch.uint8, device="cuda:0")
            dsizes = torch.full((len(sizes),), -9, dtype=torch.int32, device="cuda:0")
            dg.decompress_data_accumulate(rows, accs, accumulate, None, status, dsizes, prob_bits, dtype, _factor(mode, inv))
            assert status.tolist() == [1] * len(sizes) and dsizes.tolist() == sizes
            for i in range(len(sizes)):
                assert np.array_equal(plain[i].cpu().numpy(), data[i][1]), i
                ref = torch.from_numpy(data[i][1]).view(dtype).float() * torch.tensor(inv[i], dtype=torch.float32)
                ref = start[i] + ref if accumulate else ref
                nan = torch.isnan(ref).numpy()
                assert np.array_equal(torch.isnan(accs[i]).cpu().numpy(), nan), i
                assert np.array_equal(_u32(accs[i])[~nan], _u32(ref)[~nan]), (i, accumulate)
    finally:
        dg.prefer_torch_ops(True)


@pytest.mark.parametrize("fault", ["truncated", "capacity"])
@pytest.mark.parametrize("dtype", [E4, E5], ids=["e4m3fn", "e5m2"])
def test_a_failing_member_keeps_its_accumulator_and_nothing_else_is_written(fault, dtype):
    sizes, gap = [4097, 16 * BLK + 17, 5001, 31], 3
    data = [_case("grad", dtype, n, i, 64.0) for i, n in enumerate(sizes)]
    comp, csizes, _ = dg.compress_data_cast([_gpu(x) for x, _ in data], dtype, scale=64.0)
    rows = [comp[i, : int(csizes[i])] for i in range(len(sizes))]
    caps = list(sizes)
    if fault == "truncated":
        rows[1] = rows[1][: rows[1].numel() - 16]
    else:
        caps[1] -= 1  # the accumulator one word short
    flat = torch.full((4 * (sum(sizes) + gap * (len(sizes) + 1)),), 0xA5, dtype=torch.uint8, device="cuda:0").view(torch.float32)
    at = np.cumsum([gap] + [n + gap for n in sizes[:-1]]).tolist()
    status = torch.full((len(sizes),), 9, dtype=torch.uint8, device="cuda:0")
    dg.decompress_data_accumulate(rows, [flat[a : a + c] for a, c in zip(at, caps)], False, None, status, None, dtype=dtype, scale=0.25)
    want = np.full(flat.numel(), 0xA5A5A5A5, dtype=np.uint32).view(np.int32)
    for i, (a, n) in enumerate(zip(at, sizes)):
        if i != 1:
            want[a : a + n] = _u32(torch.from_numpy(data[i][1]).view(dtype).float() * 0.25)
    assert status.tolist() == [1, 0, 1, 1] and np.array_equal(_u32(flat), want)
