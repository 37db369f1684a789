"""compressed_all_reduce on CPU: two gloo ranks reduce-scatter compressed shards into float32, cast-compress their shard
of the sum back to bfloat16 and all-gather the archives.  The per-rank codec here is the CPU oracle (test
infrastructure), its compress_cast the reference conversion of tests/cast_ref.py followed by the oracle's compress: what
is under test is the plumbing -- which shard goes where, the order of the sum, ONE rounding, the same bits on every rank."""
import os
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

from test_accumulate_gloo import ROOT, WORDS, _OracleAccumCodec, _free_port, _tensor_of


class _OracleAllReduceCodec(_OracleAccumCodec):
    def compress_cast(self, tensors, dtype):
        import cast_ref as R

        assert dtype == torch.bfloat16 and all(t.dtype == torch.float32 for t in tensors)
        rounded = [torch.from_numpy(R.cast_ref(t.contiguous().numpy().view(np.uint32), R.BFLOAT16).view(np.int16)).view(torch.bfloat16)
                   for t in tensors]
        return self.compress(rounded)

    def decompress(self, rows, outs):
        O = self.O
        for r, out in zip(rows, outs):
            rc, w, _ = O.float_decompress(O.BFLOAT16, r.numpy(), 10, out.numel())
            assert rc == 0 and w.size == out.numel()
            out.view(torch.int16).copy_(torch.from_numpy(w.view(np.int16).copy()))
        return torch.ones((len(rows),), dtype=torch.uint8)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import oracle as O
    from dietgpu_amd import distributed as D

    D.init(backend="gloo")
    x = _tensor_of(rank, world)
    before = x.clone()
    out, stats = D.compressed_all_reduce(x, codec=_OracleAllReduceCodec(O))
    dist.barrier()
    assert torch.equal(x.view(torch.int16), before.view(torch.int16))
    q.put((rank, out.dtype == torch.bfloat16, out.view(torch.int16).numpy().view(np.uint16).copy(), stats))
    dist.destroy_process_group()


def test_compressed_all_reduce_world2():
    import cast_ref as R

    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    inputs = [_tensor_of(r, world) for r in range(world)]
    # the sequential float32 sum in rank order of the exactly widened inputs, rounded once
    total = (inputs[0].to(torch.float32).numpy() + inputs[1].to(torch.float32).numpy()).astype(np.float32)
    want = R.cast_ref(total.view(np.uint32), R.BFLOAT16)
    for rank, is_bf16, words, stats in res:
        assert is_bf16 and words.shape == (world * WORDS,)
        assert np.array_equal(words, want), f"rank {rank}: the reduced tensor differs"
        assert stats["raw_bytes"] == world * WORDS * 2 + WORDS * 2  # the reduce-scatter's rows and the gathered shard
        assert stats["wire_bytes"] < stats["raw_bytes"] and stats["payload_bytes"] < stats["raw_bytes"]


def test_compressed_all_reduce_takes_16_bit_tensors_only():
    from dietgpu_amd import distributed as D

    import pytest

    with pytest.raises(RuntimeError):
        D.compressed_all_reduce(torch.zeros(16, dtype=torch.float32), codec=object())
