"""The eight reduce calls as one family: every combination of {reduce-compress or decode-reduce} x {a raw row among the
sources or not} x {scale None, 1/3} x {norm outputs none, both}, each on the ctypes route and on the torch route, on one
batch.  The per-feature tests were each written for their own rung of the ladder; this one is for the dispatch between
them (ops._reduce_call, torch_ops.cpp reduceCall, capi.hip ReduceOptions / reduceForm).

The batch: three members of two sources each, 8185 words (two blocks, the second partial), 70000 words (two 16-block
tiles) and 4096 words; +inf planted in member 0; the second source of member 2 is an archive of the OTHER 16-bit type,
so that member must fail.  With "a raw row", the first source of member 1 is passed uncompressed.

Expected values are arithmetic, not the library's: the sources are archives of known tensors and the codec is lossless,
so the accumulator is ((old + x0) + x1) in float32 on the CPU, times fl32(scale) in float32; the archive decodes to that
rounded to the dtype (torch on the CPU: nearest even, overflow to infinity); out_nonfinite is the exact count and
out_sumsq the exact float64 sum of squares of the finite words (tests/norm_ref.py) within the bound the docstring of
decompress_data_reduce states, words * 2**-52.  The failed member keeps every bit of its accumulator and gets status 0,
0.0 and 0.  The two routes must agree bit for bit."""
import functools
import itertools

import pytest
import torch

import norm_ref as N

pytestmark = pytest.mark.gpu

SIZES = (8185, 70000, 4096)
FAILS = 2  # the member whose second source is of the wrong type
RAW_AT = (1, 0)  # (member, source) passed as a raw row
THIRD = 1.0 / 3.0
OTHER = {torch.bfloat16: torch.float16, torch.float16: torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _batch(dtype):
    """-> (old accumulators, sources x[s][i], archives of them as rows on the GPU; member FAILS: of the other type) -- on
    the CPU but for the rows, made once and never written"""
    import dietgpu_amd as dg

    g = torch.Generator().manual_seed(1234 + (dtype == torch.float16))
    old = [torch.randn(n, generator=g) * 3.0 for n in SIZES]
    x = [[(torch.randn(n, generator=g) * 2.0).to(dtype) for n in SIZES] for _ in range(2)]
    x[0][0][5000] = float("inf")
    rows = []
    for s in range(2):
        gpu = [t.cuda() for t in x[s]]
        if s == 1:
            gpu[FAILS] = gpu[FAILS].to(OTHER[dtype])
        per_type = []
        for t in gpu:  # (one call per tensor: a call compresses one float type)
            comp, sizes, _ = dg.compress_data(True, [t], False)
            per_type.append(comp[0, : int(sizes[0])].clone())
        rows.append(per_type)
    torch.cuda.synchronize()
    return old, x, rows


def _expected(dtype, compress, scale):
    """-> per member (accumulator words, the words the norm outputs measure, archive words or None)"""
    old, x, _ = _batch(dtype)
    out = []
    for i in range(len(SIZES)):
        if i == FAILS:
            out.append((old[i], None, old[i].to(dtype) if compress else None))
            continue
        acc = (old[i] + x[0][i].float()) + x[1][i].float()
        if scale is not None:
            acc = acc * torch.tensor(scale, dtype=torch.float32)  # (fl32(scale), one float32 multiply)
        arch = acc.to(dtype) if compress else None
        out.append((acc, arch.float() if compress else acc, arch))
    return out


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _run(dtype, compress, raw, scale, norm, torch_route):
    import dietgpu_amd as dg

    old, x, rows = _batch(dtype)
    n = len(SIZES)
    ins = [[rows[s][i] for s in range(2)] for i in range(n)]
    if raw:
        ins[RAW_AT[0]][RAW_AT[1]] = x[RAW_AT[1]][RAW_AT[0]].cuda()
    accs = [t.cuda() for t in old]
    status = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    kw = {"dtype": dtype, "scale": scale}
    if norm:
        kw["out_sumsq"] = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
        kw["out_nonfinite"] = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    name = "decompress_data_reduce" + ("_compress" if compress else "") + ("_mixed" if raw else "")
    dg.ops.prefer_torch_ops(torch_route)
    try:
        assert (dg.ops._fast_ops(10) is not None) == torch_route, "the torch route is not there"
        out = getattr(dg, name)(ins, accs, True, None, status, sizes, **kw)
        archives = None
        if compress:
            comp, csizes, _ = out
            host = csizes.tolist()
            archives = [comp[i, : host[i]] for i in range(n)]
            decoded = [torch.empty(SIZES[i], dtype=dtype, device="cuda") for i in range(n)]
            dg.decompress_data(True, archives, decoded, False)
            archives = [a.cpu() for a in archives]
            decoded = [d.cpu() for d in decoded]
    finally:
        dg.ops.prefer_torch_ops(True)
    got = {"acc": [a.cpu() for a in accs], "status": status.tolist(), "sizes": sizes.tolist(), "archives": archives,
           "decoded": decoded if compress else None}
    if norm:
        got["sumsq"], got["nonfinite"] = kw["out_sumsq"].cpu(), kw["out_nonfinite"].tolist()
    return got


def _check(dtype, compress, raw, scale, norm):
    what = f"{dtype} compress={compress} raw={raw} scale={scale} norm={norm}"
    want = _expected(dtype, compress, scale)
    routes = [_run(dtype, compress, raw, scale, norm, torch_route) for torch_route in (False, True)]
    for route, got in zip(("ctypes", "torch"), routes):
        assert got["status"] == [0 if i == FAILS else 1 for i in range(len(SIZES))], (what, route)
        assert got["sizes"] == list(SIZES), (what, route)
        for i, (acc, measured, arch) in enumerate(want):
            assert torch.equal(_bits(got["acc"][i]), _bits(acc)), f"{what} {route}: accumulator {i}"
            if compress:
                assert torch.equal(_bits(got["decoded"][i]), _bits(arch)), f"{what} {route}: archive {i}"
            if norm and i == FAILS:
                assert got["sumsq"][i].item() == 0.0 and got["nonfinite"][i] == 0, f"{what} {route}: failed member {i}"
            elif norm:
                N.check(got["sumsq"][i].item(), got["nonfinite"][i], measured.numpy(), f"{what} {route}: member {i}")
        if norm:
            assert got["nonfinite"][0] >= 1, f"{what} {route}: the planted inf"
    a, b = routes
    assert a["status"] == b["status"] and a["sizes"] == b["sizes"], what
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a["acc"], b["acc"])), f"{what}: accumulators differ between the routes"
    if compress:
        assert all(torch.equal(p, q) for p, q in zip(a["archives"], b["archives"])), f"{what}: archives differ between the routes"
    if norm:
        assert torch.equal(a["sumsq"].view(torch.int64), b["sumsq"].view(torch.int64)) and a["nonfinite"] == b["nonfinite"], what


COMBINATIONS = list(itertools.product((False, True), (False, True), (None, THIRD), (False, True)))


@pytest.mark.parametrize("compress,raw,scale,norm", COMBINATIONS)
def test_every_combination_on_both_routes_bfloat16(compress, raw, scale, norm):
    _check(torch.bfloat16, compress, raw, scale, norm)


@pytest.mark.parametrize("raw,scale,norm", [c[1:] for c in COMBINATIONS if c[0]])
def test_every_reduce_compress_combination_on_both_routes_float16(raw, scale, norm):
    _check(torch.float16, True, raw, scale, norm)
