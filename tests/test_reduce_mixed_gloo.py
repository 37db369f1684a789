"""raw_local of compressed_reduce_scatter / compressed_all_reduce on CPU: two gloo ranks, and a per-rank codec that is
the CPU oracle (numpy widening and float32 adds, oracle.float_compress / float_decompress) and logs every call.  What is
under test is the plumbing: with raw_local=True the rank's own shard is not compressed (`compress` gets world - 1
tensors), travels nowhere, and enters ONE mixed call uncompressed at position `rank` of the rank order; a codec without
the mixed methods takes today's path call for call, as raw_local=False does; and every variant returns the same bits,
the same on both ranks."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_accumulate_gloo import ROOT, WORDS, _free_port, _tensor_of

WORLD = 2


def _codecs(O):
    import cast_ref

    class Plain:
        """compress, decompress, decompress_accumulate, compress_cast: the three-step paths"""

        def __init__(self):
            self.log = []

        def _archive_rows(self, tensors):
            arch = [O.float_compress(O.BFLOAT16, t.contiguous().view(torch.int16).numpy().view(np.uint16), 10) for t in tensors]
            cap = max(O.float_max_compressed_size(O.BFLOAT16, t.numel()) for t in tensors)
            comp = torch.zeros((len(arch), cap), dtype=torch.uint8)
            for i, a in enumerate(arch):
                comp[i, : a.size] = torch.from_numpy(a.copy())
            return comp, torch.tensor([a.size for a in arch], dtype=torch.int32)

        @staticmethod
        def _wide(row, n):
            """the exact float32 widening of a source: an archive is decoded, a raw bf16 row taken as it is"""
            if row.dtype == torch.uint8:
                rc, w, _ = O.float_decompress(O.BFLOAT16, row.numpy(), 10, n)
                assert rc == 0 and w.size == n
            else:
                assert row.dtype == torch.bfloat16 and row.dim() == 1 and row.numel() == n
                w = row.contiguous().view(torch.int16).numpy().view(np.uint16)
            return (w.astype(np.uint32) << 16).view(np.float32)

        def _sum(self, rows, acc, accumulate):
            a = acc.numpy()
            for k, r in enumerate(rows):
                wide = self._wide(r, acc.numel())
                a[:] = (a + wide).astype(np.float32) if (accumulate or k > 0) else wide

        def compress(self, tensors):
            self.log.append(("compress", len(tensors)))
            return self._archive_rows(tensors)

        def compress_cast(self, tensors, dtype):
            self.log.append(("compress_cast", len(tensors)))
            assert dtype == torch.bfloat16
            rounded = [torch.from_numpy(cast_ref.cast_ref(t.contiguous().numpy().view(np.uint32), cast_ref.BFLOAT16).view(np.int16))
                       .view(torch.bfloat16) for t in tensors]
            return self._archive_rows(rounded)

        def decompress(self, rows, outs):
            self.log.append(("decompress", len(rows)))
            for r, out in zip(rows, outs):
                rc, w, _ = O.float_decompress(O.BFLOAT16, r.numpy(), 10, out.numel())
                assert rc == 0 and w.size == out.numel()
                out.view(torch.int16).copy_(torch.from_numpy(w.view(np.int16).copy()))
            return torch.ones((len(rows),), dtype=torch.uint8)

        def decompress_accumulate(self, rows, accs, accumulate):
            self.log.append(("decompress_accumulate", [str(r.dtype) for r in rows], bool(accumulate)))
            for r, acc in zip(rows, accs):
                self._sum([r], acc, accumulate)
            return torch.ones((len(rows),), dtype=torch.uint8)

    class Mixed(Plain):
        """... and decompress_reduce_mixed: the reduce-scatter sums in one call"""

        def decompress_reduce_mixed(self, rows_per_acc, accs, accumulate):
            self.log.append(("decompress_reduce_mixed", [[str(r.dtype) for r in rows] for rows in rows_per_acc], bool(accumulate)))
            for rows, acc in zip(rows_per_acc, accs):
                self._sum(rows, acc, accumulate)
            return torch.ones((len(accs),), dtype=torch.uint8)

    class Fused(Plain):
        """the one-call middle of the all-reduce, archives only"""

        def decompress_reduce_compress(self, rows_per_acc, accs, accumulate):
            self.log.append(("decompress_reduce_compress", [[str(r.dtype) for r in rows] for rows in rows_per_acc], bool(accumulate)))
            for rows, acc in zip(rows_per_acc, accs):
                self._sum(rows, acc, accumulate)
            comp, sizes = Plain.compress_cast(self, accs, torch.bfloat16)
            self.log.pop()
            return torch.ones((len(accs),), dtype=torch.uint8), comp, sizes

    class FusedMixed(Fused, Mixed):
        def decompress_reduce_compress_mixed(self, rows_per_acc, accs, accumulate):
            self.log.append(("decompress_reduce_compress_mixed", [[str(r.dtype) for r in rows] for rows in rows_per_acc], bool(accumulate)))
            for rows, acc in zip(rows_per_acc, accs):
                self._sum(rows, acc, accumulate)
            comp, sizes = Plain.compress_cast(self, accs, torch.bfloat16)
            self.log.pop()
            return torch.ones((len(accs),), dtype=torch.uint8), comp, sizes

    return {"Plain": Plain, "Mixed": Mixed, "Fused": Fused, "FusedMixed": FusedMixed}


# (collective, codec, raw_local)
RUNS = [("reduce_scatter", "Mixed", True), ("reduce_scatter", "Mixed", False), ("reduce_scatter", "Plain", True),
        ("all_reduce", "FusedMixed", True), ("all_reduce", "FusedMixed", False), ("all_reduce", "Fused", True),
        ("all_reduce", "Mixed", True), ("all_reduce", "Plain", True)]


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import oracle as O
    from dietgpu_amd import distributed as D

    D.init(backend="gloo")
    codecs = _codecs(O)
    out = []
    for collective, name, raw_local in RUNS:
        codec = codecs[name]()
        x = _tensor_of(rank, world)
        before = x.clone()
        if collective == "reduce_scatter":
            res, stats = D.compressed_reduce_scatter(x, codec=codec, raw_local=raw_local)
            bits = res.numpy().view(np.uint32).copy()
        else:
            res, stats = D.compressed_all_reduce(x, codec=codec, raw_local=raw_local)
            bits = res.view(torch.int16).numpy().view(np.uint16).copy()
        assert torch.equal(x.view(torch.int16), before.view(torch.int16))
        out.append((bits, stats, codec.log))
    dist.barrier()
    q.put((rank, out))
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def results():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(WORLD))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def _run(results, rank, collective, name, raw_local):
    return results[rank][RUNS.index((collective, name, raw_local))]


U8, BF = "torch.uint8", "torch.bfloat16"


def _kinds(rank):
    """the sources of rank's shard in rank order, its own one raw"""
    return [BF if r == rank else U8 for r in range(WORLD)]


def test_reduce_scatter_raw_local_compresses_the_other_shards_and_makes_one_mixed_call(results):
    for rank in range(WORLD):
        _, stats, log = _run(results, rank, "reduce_scatter", "Mixed", True)
        assert log == [("compress", WORLD - 1), ("decompress_reduce_mixed", [_kinds(rank)], False)], f"rank {rank}: {log}"
        _, plain_stats, _ = _run(results, rank, "reduce_scatter", "Mixed", False)
        # the own row is no longer part of the payload; the other row is the one the default path sends
        assert 0 < stats["payload_bytes"] < plain_stats["payload_bytes"]
        assert stats["raw_bytes"] == plain_stats["raw_bytes"] == WORLD * WORDS * 2


def test_reduce_scatter_default_and_a_codec_without_the_method_take_todays_path(results):
    today = [("compress", WORLD)] + [("decompress_accumulate", [U8], r != 0) for r in range(WORLD)]
    for rank in range(WORLD):
        assert _run(results, rank, "reduce_scatter", "Mixed", False)[2] == today
        assert _run(results, rank, "reduce_scatter", "Plain", True)[2] == today


def test_reduce_scatter_bits_do_not_depend_on_raw_local(results):
    inputs = [_tensor_of(r, WORLD).to(torch.float32).numpy().reshape(WORLD, WORDS) for r in range(WORLD)]
    for rank in range(WORLD):
        want = (inputs[0][rank] + inputs[1][rank]).astype(np.float32).view(np.uint32)
        for name, raw_local in (("Mixed", True), ("Mixed", False), ("Plain", True)):
            assert np.array_equal(_run(results, rank, "reduce_scatter", name, raw_local)[0], want), (rank, name, raw_local)


def test_all_reduce_raw_local_makes_one_mixed_call(results):
    gather = [("decompress", 1)] * WORLD
    for rank in range(WORLD):
        _, stats, log = _run(results, rank, "all_reduce", "FusedMixed", True)
        assert log == [("compress", WORLD - 1), ("decompress_reduce_compress_mixed", [_kinds(rank)], False)] + gather, f"rank {rank}: {log}"
        _, plain_stats, plain_log = _run(results, rank, "all_reduce", "FusedMixed", False)
        today = [("compress", WORLD), ("decompress_reduce_compress", [[U8] * WORLD], False)] + gather
        assert plain_log == today, f"rank {rank}: {plain_log}"
        assert _run(results, rank, "all_reduce", "Fused", True)[2] == today  # no mixed method: today's path, quietly
        assert 0 < stats["payload_bytes"] < plain_stats["payload_bytes"]
        # the three-step path: the reduce-scatter's mixed call when the codec has that one
        assert _run(results, rank, "all_reduce", "Mixed", True)[2] == [
            ("compress", WORLD - 1), ("decompress_reduce_mixed", [_kinds(rank)], False), ("compress_cast", 1)] + gather
        assert _run(results, rank, "all_reduce", "Plain", True)[2] == (
            [("compress", WORLD)] + [("decompress_accumulate", [U8], r != 0) for r in range(WORLD)] + [("compress_cast", 1)] + gather)


def test_all_reduce_bits_do_not_depend_on_raw_local_or_the_rank(results):
    import cast_ref

    inputs = [_tensor_of(r, WORLD).to(torch.float32).numpy() for r in range(WORLD)]
    want = cast_ref.cast_ref((inputs[0] + inputs[1]).astype(np.float32).view(np.uint32), cast_ref.BFLOAT16)
    for rank in range(WORLD):
        for name, raw_local in (("FusedMixed", True), ("FusedMixed", False), ("Fused", True), ("Mixed", True), ("Plain", True)):
            assert np.array_equal(_run(results, rank, "all_reduce", name, raw_local)[0], want), (rank, name, raw_local)
