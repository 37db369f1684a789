"""norm= of compressed_reduce_scatter / compressed_all_reduce on CPU: two gloo ranks, the CPU oracle as the per-rank codec
(test infrastructure).  What is under test is the plumbing: with norm=False the codec is called with exactly the
arguments it gets today; a codec whose methods have a `norm` parameter is handed the (sumsq, nonfinite) pair once; a
codec without one gets the statistic from one torch pass -- over the float32 shard in the reduce-scatter, over the shard
rounded to the input dtype in the all-reduce.  Both ways give the same non-finite count and a squared norm within
n * 2**-52 of the exact one (tests/norm_ref.py), and global_sumsq / global_nonfinite describe the tensor
compressed_all_reduce returns, the same on both ranks.

The inputs hold a word whose float32 sum overflows, an infinity, and a word whose float32 sum is finite and rounds to a
bfloat16 infinity: the reduce-scatter counts two non-finite words, the all-reduce three."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import norm_ref as N
from test_accumulate_gloo import ROOT, WORDS, _free_port, _tensor_of

KINDS = ("norm in the codec", "no norm in the codec", "norm but no scale in the codec")
UNSET = "no keyword"


def _inputs(rank, world):
    x = _tensor_of(rank, world)
    x[7] = 3.0e38  # both ranks: the float32 sum is +inf
    if rank == 1:
        x[WORDS + 3] = float("-inf")
    # the largest bfloat16 and 1e36: a finite float32 sum past the tie to the bfloat16 infinity
    x[WORDS + 100] = torch.tensor([0x7F7F], dtype=torch.int16).view(torch.bfloat16)[0] if rank == 0 else 1.0e36
    return x


def _worker(rank, world, port, q, kind):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import norm_ref
    import oracle as O
    from dietgpu_amd import distributed as D
    from test_all_reduce_gloo import _OracleAllReduceCodec

    class Logging(_OracleAllReduceCodec):
        def __init__(self, O):
            super().__init__(O)
            self.log = []

        def compress_cast(self, tensors, dtype):
            self.log.append(("cast",))
            return super().compress_cast(tensors, dtype)

        def _sum(self, rows_per_acc, accs, accumulate, scale, norm, rounded):
            for i, (rows, acc) in enumerate(zip(rows_per_acc, accs)):
                for k, r in enumerate(rows):
                    _OracleAllReduceCodec.decompress_accumulate(self, [r], [acc], accumulate or k > 0)
                a = acc.numpy()
                if scale is not UNSET and scale is not None:
                    with np.errstate(over="ignore", invalid="ignore"):
                        a[:] = (a * np.float32(scale)).astype(np.float32)
                if norm is not UNSET and norm is not None:
                    sq, bad, _ = norm_ref.stats(norm_ref.rounded(a, torch.bfloat16) if rounded else a)
                    norm[0][i], norm[1][i] = sq, bad
            return torch.ones((len(accs),), dtype=torch.uint8)

        @staticmethod
        def _seen(norm):
            return norm if norm is UNSET or norm is None else tuple((t.dtype, tuple(t.shape)) for t in norm)

    class WithNorm(Logging):
        def decompress_reduce(self, rows_per_acc, accs, accumulate, scale=UNSET, norm=UNSET):
            self.log.append(("reduce", [len(r) for r in rows_per_acc], bool(accumulate), scale, self._seen(norm)))
            return self._sum(rows_per_acc, accs, accumulate, scale, norm, False)

        def decompress_reduce_compress(self, rows_per_acc, accs, accumulate, scale=UNSET, norm=UNSET):
            self.log.append(("fused", [len(r) for r in rows_per_acc], bool(accumulate), scale, self._seen(norm)))
            status = self._sum(rows_per_acc, accs, accumulate, scale, norm, True)
            comp, sizes = _OracleAllReduceCodec.compress_cast(self, accs, torch.bfloat16)
            return status, comp, sizes

    class WithoutNorm(Logging):
        def decompress_reduce(self, rows_per_acc, accs, accumulate, scale=UNSET):
            self.log.append(("reduce", [len(r) for r in rows_per_acc], bool(accumulate), scale, UNSET))
            return self._sum(rows_per_acc, accs, accumulate, scale, UNSET, False)

        def decompress_reduce_compress(self, rows_per_acc, accs, accumulate, scale=UNSET):
            self.log.append(("fused", [len(r) for r in rows_per_acc], bool(accumulate), scale, UNSET))
            status = self._sum(rows_per_acc, accs, accumulate, scale, UNSET, True)
            comp, sizes = _OracleAllReduceCodec.compress_cast(self, accs, torch.bfloat16)
            return status, comp, sizes

    class NormButNoScale(Logging):  # (a factor is then applied AFTER the codec's call: its norm would be that of the unscaled sum)
        def decompress_reduce(self, rows_per_acc, accs, accumulate, norm=UNSET):
            self.log.append(("reduce", [len(r) for r in rows_per_acc], bool(accumulate), UNSET, self._seen(norm)))
            return self._sum(rows_per_acc, accs, accumulate, UNSET, norm, False)

    D.init(backend="gloo")
    make = {KINDS[0]: WithNorm, KINDS[1]: WithoutNorm, KINDS[2]: NormButNoScale}[kind]
    x = _inputs(rank, world)
    before = x.clone()
    results = {}
    for name, kw in (("sum", {}), ("avg", {"op": "avg"})):
        for norm in (False, True):
            codec = make(O)
            out, stats = D.compressed_all_reduce(x, codec=codec, norm=norm, **kw)
            results["all-reduce", name, norm] = (out.to(torch.float32).numpy().copy(), {k: v.clone() for k, v in stats.items() if torch.is_tensor(v)},
                                                  sorted(stats), codec.log)
            codec = make(O)
            shard, stats = D.compressed_reduce_scatter(x, codec=codec, norm=norm, **kw)
            results["reduce-scatter", name, norm] = (shard.numpy().copy(), {k: v.clone() for k, v in stats.items() if torch.is_tensor(v)}, sorted(stats),
                                                      codec.log)
    dist.barrier()
    assert torch.equal(x.view(torch.int16), before.view(torch.int16))
    q.put((rank, results))
    dist.destroy_process_group()


@pytest.mark.parametrize("kind", KINDS)
def test_norm_on_every_codec_path(kind):
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, kind)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    inputs = [_inputs(r, world) for r in range(world)]
    with np.errstate(over="ignore", invalid="ignore"):
        total = (inputs[0].to(torch.float32).numpy() + inputs[1].to(torch.float32).numpy()).astype(np.float32)
    pair = ((torch.float64, (1,)), (torch.int32, (1,)))
    base = ["payload_bytes", "raw_bytes", "wire_bytes"]
    seen_global = {}
    for rank, results in sorted(res):
        for name, f in (("sum", None), ("avg", 0.5)):
            with np.errstate(over="ignore", invalid="ignore"):
                whole = total if f is None else (total * np.float32(f)).astype(np.float32)
            shard = whole[rank * WORDS : (rank + 1) * WORDS]
            factor = UNSET if f is None else f
            # ---- norm=False: the calls and the stats of today
            out, tensors, keys, log = results["all-reduce", name, False]
            assert keys == base and tensors == {}, (kind, name, keys)
            if kind == KINDS[2]:
                assert log == [("reduce", [world], False, UNSET, UNSET), ("cast",)]
            else:
                assert log == [("fused", [world], False, factor, UNSET)]
            _, tensors, keys, log = results["reduce-scatter", name, False]
            assert keys == base and tensors == {}
            assert log == [("reduce", [world], False, UNSET if kind == KINDS[2] else factor, UNSET)]
            # ---- reduce-scatter with norm=True: the float32 shard
            got, tensors, keys, log = results["reduce-scatter", name, True]
            assert keys == sorted(base + ["sumsq", "nonfinite"]), keys
            assert np.array_equal(got.view(np.uint32), shard.view(np.uint32))
            handed = kind == KINDS[0] or (kind == KINDS[2] and f is None)
            assert log == [("reduce", [world], False, UNSET if kind == KINDS[2] else factor, pair if handed else UNSET)], (kind, name, log)
            assert tensors["sumsq"].dtype == torch.float64 and tensors["sumsq"].dim() == 0
            assert tensors["nonfinite"].dtype == torch.int32 and tensors["nonfinite"].dim() == 0
            N.check(float(tensors["sumsq"]), int(tensors["nonfinite"]), shard, f"{kind}, rank {rank}, reduce-scatter {name}")
            # ---- all-reduce with norm=True: the shard rounded to bfloat16, and the whole returned tensor
            out, tensors, keys, log = results["all-reduce", name, True]
            assert keys == sorted(base + ["sumsq", "nonfinite", "global_sumsq", "global_nonfinite"]), keys
            assert np.array_equal(out.view(np.uint32), N.rounded(whole, torch.bfloat16).view(np.uint32))
            if kind == KINDS[2]:
                assert log == [("reduce", [world], False, UNSET, UNSET), ("cast",)]  # (the float32 shard's norm is not the archive's)
            else:
                assert log == [("fused", [world], False, factor, pair if kind == KINDS[0] else UNSET)], (kind, name, log)
            N.check(float(tensors["sumsq"]), int(tensors["nonfinite"]), N.rounded(shard, torch.bfloat16), f"{kind}, rank {rank}, all-reduce {name}")
            assert tensors["global_sumsq"].dtype == torch.float64 and tensors["global_sumsq"].dim() == 0
            assert tensors["global_nonfinite"].dtype == torch.int32 and tensors["global_nonfinite"].dim() == 0
            N.check(float(tensors["global_sumsq"]), int(tensors["global_nonfinite"]), out, f"{kind}, rank {rank}, all-reduce {name}: the returned tensor")
            both = (float(tensors["global_sumsq"]), int(tensors["global_nonfinite"]))
            assert seen_global.setdefault(name, both) == both, f"{kind} {name}: the ranks disagree"
        # the sum: one overflow in rank 0's shard; an infinity in rank 1's, and there the word that only the rounding makes infinite
        assert int(results["reduce-scatter", "sum", True][1]["nonfinite"]) == 1
        assert int(results["all-reduce", "sum", True][1]["nonfinite"]) == (1 if rank == 0 else 2)
        assert int(results["all-reduce", "sum", True][1]["global_nonfinite"]) == 3
