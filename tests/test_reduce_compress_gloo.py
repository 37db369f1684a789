"""compressed_all_reduce with a codec that has decompress_reduce_compress, on CPU: two gloo ranks exchange compressed
shards, and the middle of the collective -- sum of the received rows, archive of the rounded sum -- is ONE codec call.
The per-rank codec is the CPU oracle (test infrastructure): what is under test is the plumbing -- that the one call is
made, exactly once and with the rows in rank order, that a codec without it takes the three-step path as before, and
that both give the float32 sum in rank order rounded once, the same bits on every rank."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_accumulate_gloo import ROOT, WORDS, _free_port, _tensor_of


def _worker(rank, world, port, q, one_call):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import oracle as O
    from dietgpu_amd import distributed as D
    from test_all_reduce_gloo import _OracleAllReduceCodec

    class Counting(_OracleAllReduceCodec):
        """counts the calls of the middle of the collective"""

        def __init__(self, O):
            super().__init__(O)
            self.fused, self.accumulates, self.casts = [], 0, 0

        def decompress_accumulate(self, rows, accs, accumulate):
            self.accumulates += 1
            return super().decompress_accumulate(rows, accs, accumulate)

        def compress_cast(self, tensors, dtype):
            self.casts += 1
            return super().compress_cast(tensors, dtype)

    class Fused(Counting):
        def decompress_reduce_compress(self, rows_per_acc, accs, accumulate):
            self.fused.append(([len(rows) for rows in rows_per_acc], len(accs), bool(accumulate)))
            for rows, acc in zip(rows_per_acc, accs):
                for k, r in enumerate(rows):
                    _OracleAllReduceCodec.decompress_accumulate(self, [r], [acc], accumulate or k > 0)
            comp, sizes = _OracleAllReduceCodec.compress_cast(self, accs, torch.bfloat16)
            return torch.ones((len(accs),), dtype=torch.uint8), comp, sizes

    D.init(backend="gloo")
    codec = (Fused if one_call else Counting)(O)
    x = _tensor_of(rank, world)
    out, stats = D.compressed_all_reduce(x, codec=codec)
    dist.barrier()
    q.put((rank, out.view(torch.int16).numpy().view(np.uint16).copy(), stats, codec.fused, codec.accumulates, codec.casts))
    dist.destroy_process_group()


@pytest.mark.parametrize("one_call", [True, False])
def test_compressed_all_reduce_middle_is_one_call_when_the_codec_has_it(one_call):
    import cast_ref as R

    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, one_call)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    inputs = [_tensor_of(r, world) for r in range(world)]
    total = (inputs[0].to(torch.float32).numpy() + inputs[1].to(torch.float32).numpy()).astype(np.float32)
    want = R.cast_ref(total.view(np.uint32), R.BFLOAT16)
    for rank, words, stats, fused, accumulates, casts in res:
        if one_call:
            assert fused == [([world], 1, False)], f"rank {rank}: one call with `world` rows, accumulate off"
            assert accumulates == 0 and casts == 0, f"rank {rank}: the three-step path ran beside the one call"
        else:
            assert fused == [] and accumulates == world and casts == 1, f"rank {rank}: not the three-step path"
        assert np.array_equal(words, want), f"rank {rank}: the reduced tensor differs"
        assert stats["raw_bytes"] == world * WORDS * 2 + WORDS * 2  # the same accounting on both paths
        assert stats["wire_bytes"] < stats["raw_bytes"] and stats["payload_bytes"] < stats["raw_bytes"]
