"""norm=True of compressed_all_reduce / compressed_reduce_scatter with the default codec, on one device.

World 2 (two processes on device 0, backend gloo, as bench.py's two-rank runs): every shard is the sum of two sources, an
archive and -- with raw_local -- the rank's own uncompressed row; per rank `sumsq` / `nonfinite` are checked against
tests/norm_ref.py (the float32 shard for the reduce-scatter, the shard rounded to the dtype for the all-reduce),
`global_sumsq` / `global_nonfinite` against the tensor the call returns, and both ranks must report the same global pair.

World 1 on RCCL: the pair
reaches the reduce kernel on the one-call path (reduce-compress: the words of the archive are measured), on the
reduce-scatter (decode-reduce: the float32 shard is measured) and with raw_local=True; on the three-step path, and with a
codec whose methods have no `norm` parameter, one torch pass gives the same count and a squared norm within the bound.
The sum of one rank's tensor is the tensor, scaled by 2: a float16 word of 40000 is 80000.0f in the float32 shard,
finite, and +inf in the returned tensor."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import cast_ref as R
import norm_ref as N
from test_gpu_reduce_scaled_all_reduce import WORDS, _free_port

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype,ft", [(torch.bfloat16, R.BFLOAT16), (torch.float16, R.FLOAT16)])
def test_norm_reaches_the_kernel_on_every_path(dtype, ft):
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    dietgpu_amd.lib()
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    D.init(backend="nccl", device=dev)  # "nccl" is RCCL on ROCm
    try:
        g = torch.Generator(device="cpu").manual_seed(31)
        mine = torch.randn(WORDS, generator=g).to(dtype)
        mine[5] = float("inf")
        mine[4096 + 7] = float("nan")
        mine[3 * 4096] = 40000.0  # (bfloat16: 39936)
        x = mine.to(dev)
        words = mine.view(torch.int16).numpy().view(np.uint16)
        with np.errstate(invalid="ignore"):
            shard_want = (R.widen(words, ft).view(np.float32) * np.float32(2.0)).astype(np.float32)
        out_want = N.rounded(shard_want, dtype)
        assert N.stats(shard_want)[1] == 2 and N.stats(out_want)[1] == (3 if dtype == torch.float16 else 2)

        def check(stats, words_want, what, keys):
            assert sorted(k for k in stats if k not in ("raw_bytes", "wire_bytes", "payload_bytes")) == sorted(keys), (what, sorted(stats))
            for k in keys:
                t = stats[k]
                assert t.dim() == 0 and t.device.type == "cuda" and t.dtype == (torch.int32 if "nonfinite" in k else torch.float64), (what, k)
            N.check(float(stats["sumsq"]), int(stats["nonfinite"]), words_want, f"{dtype} {what}")
            if "global_sumsq" in keys:  # a world of one: the shard is the tensor
                assert float(stats["global_sumsq"]) == float(stats["sumsq"]) and int(stats["global_nonfinite"]) == int(stats["nonfinite"]), what

        both, four = ("sumsq", "nonfinite"), ("sumsq", "nonfinite", "global_sumsq", "global_nonfinite")

        # the one-call path: the codec's own method is handed the pair, once
        fused = D.GpuFloatCodec()
        seen = []
        inner_fused = fused.decompress_reduce_compress

        def spy_fused(rows_per_acc, accs, accumulate, scale=None, norm=None):
            seen.append((scale, None if norm is None else tuple((t.dtype, tuple(t.shape)) for t in norm)))
            return inner_fused(rows_per_acc, accs, accumulate, scale=scale, norm=norm)

        fused.decompress_reduce_compress = spy_fused
        fused.decompress_reduce = fused.compress_cast = None  # (the three-step path would fail on them)
        out_one, stats_one = D.compressed_all_reduce(x, codec=fused, scale=2.0, norm=True)
        assert seen == [(2.0, ((torch.float64, (1,)), (torch.int32, (1,))))]
        assert np.array_equal(out_one.to(torch.float32).cpu().numpy().view(np.uint32)[~np.isnan(out_want)], out_want.view(np.uint32)[~np.isnan(out_want)])
        check(stats_one, out_want, "one-call path", four)

        # the three-step path (the one-call method hidden): one torch pass over the shard rounded to the dtype
        plain = D.GpuFloatCodec()
        plain.decompress_reduce_compress = None
        _, stats_three = D.compressed_all_reduce(x, codec=plain, scale=2.0, norm=True)
        check(stats_three, out_want, "three-step path", four)
        assert int(stats_three["nonfinite"]) == int(stats_one["nonfinite"])

        # raw_local: the own shard uncompressed
        _, stats_raw = D.compressed_all_reduce(x, raw_local=True, scale=2.0, norm=True)
        check(stats_raw, out_want, "raw_local, one-call path", four)

        # the reduce-scatter measures the float32 shard: 80000.0f is finite there
        shard, stats_rs = D.compressed_reduce_scatter(x, scale=2.0, norm=True)
        assert np.array_equal(shard.cpu().numpy().view(np.uint32)[~np.isnan(shard_want)], shard_want.view(np.uint32)[~np.isnan(shard_want)])
        check(stats_rs, shard_want, "reduce-scatter", both)
        _, stats_rs_raw = D.compressed_reduce_scatter(x, raw_local=True, scale=2.0, norm=True)
        check(stats_rs_raw, shard_want, "reduce-scatter, raw_local", both)

        # a codec whose method has no `norm` parameter: the torch pass
        old = D.GpuFloatCodec()
        inner_reduce = old.decompress_reduce
        old.decompress_reduce = lambda rows_per_acc, accs, accumulate, scale=None: inner_reduce(rows_per_acc, accs, accumulate, scale=scale)
        _, stats_old = D.compressed_reduce_scatter(x, codec=old, scale=2.0, norm=True)
        check(stats_old, shard_want, "reduce-scatter, a codec without norm", both)

        # without norm: the stats of today
        _, stats_none = D.compressed_all_reduce(x, scale=2.0)
        assert sorted(stats_none) == ["payload_bytes", "raw_bytes", "wire_bytes"]
        assert torch.equal(x.view(torch.int16).cpu(), mine.view(torch.int16))  # the input is unchanged
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------- two ranks
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIRD = 1.0 / 3.0
CASES = (("all-reduce", {}), ("all-reduce", {"raw_local": True}), ("all-reduce", {"raw_local": True, "scale": THIRD}), ("all-reduce", {"three_step": True}),
         ("reduce-scatter", {}), ("reduce-scatter", {"raw_local": True, "scale": THIRD}))


def _two_rank_input(rank, dtype):
    g = torch.Generator(device="cpu").manual_seed(41 + rank)
    x = torch.randn(2 * WORDS, generator=g).to(dtype)
    x[7] = 40000.0  # both ranks: 80000.0f in the float32 shard; +inf as float16, finite as bfloat16
    x[WORDS + 4096 + 3] = 40000.0
    if rank == 1:
        x[WORDS + 11] = float("-inf")
        x[3 * 4096 + 1] = float("nan")
    return x


def _two_rank_worker(rank, world, port, q, dtype):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    dietgpu_amd.lib()
    dev = torch.device("cuda:0")  # both ranks on the one device
    torch.cuda.set_device(dev)
    D.init(backend="gloo")
    try:
        x = _two_rank_input(rank, dtype).to(dev)
        results = []
        for kind, kw in CASES:
            kw = dict(kw)
            codec = D.GpuFloatCodec()
            if kw.pop("three_step", False):
                codec.decompress_reduce_compress = None
            f = D.compressed_all_reduce if kind == "all-reduce" else D.compressed_reduce_scatter
            out, stats = f(x, codec=codec, norm=True, **kw)
            torch.cuda.synchronize()
            for k, t in stats.items():
                if torch.is_tensor(t):
                    assert t.dim() == 0 and t.device.type == "cuda" and t.dtype == (torch.int32 if "nonfinite" in k else torch.float64), (kind, k)
            results.append((out.to(torch.float32).cpu().numpy(), {k: (float(v) if "sumsq" in k else int(v)) for k, v in stats.items() if torch.is_tensor(v)}))
        dist.barrier()
        q.put((rank, results))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_two_ranks_on_one_device(dtype):
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q, dtype)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    wide = [_two_rank_input(r, dtype).to(torch.float32).numpy() for r in range(world)]
    with np.errstate(invalid="ignore", over="ignore"):
        total = (wide[0] + wide[1]).astype(np.float32)  # the float32 sum in rank order
    for c, (kind, kw) in enumerate(CASES):
        with np.errstate(invalid="ignore", over="ignore"):
            whole = (total * np.float32(kw["scale"])).astype(np.float32) if "scale" in kw else total
        whole_rounded = N.rounded(whole, dtype)
        globals_seen = []
        for rank in range(world):
            out, stats = res[rank][c]
            shard = whole[rank * WORDS : (rank + 1) * WORDS]
            what = f"{dtype} {kind} {kw} rank {rank}"
            nan = np.isnan(whole)
            if kind == "reduce-scatter":
                assert sorted(stats) == ["nonfinite", "sumsq"], what
                snan = nan[rank * WORDS : (rank + 1) * WORDS]
                assert np.array_equal(out.view(np.uint32)[~snan], shard.view(np.uint32)[~snan]), what
                N.check(stats["sumsq"], stats["nonfinite"], shard, what)
            else:
                assert sorted(stats) == ["global_nonfinite", "global_sumsq", "nonfinite", "sumsq"], what
                assert np.array_equal(out.view(np.uint32)[~nan], whole_rounded.view(np.uint32)[~nan]) and np.isnan(out[nan]).all(), what
                N.check(stats["sumsq"], stats["nonfinite"], whole_rounded[rank * WORDS : (rank + 1) * WORDS], what)
                N.check(stats["global_sumsq"], stats["global_nonfinite"], out, what + ": the returned tensor")
                globals_seen.append((stats["global_sumsq"], stats["global_nonfinite"]))
        if kind == "all-reduce":
            assert globals_seen[0] == globals_seen[1], f"{dtype} {kind} {kw}: the ranks disagree"
            assert globals_seen[0][1] == (4 if dtype == torch.float16 and "scale" not in kw else 2), (dtype, kw, globals_seen)
