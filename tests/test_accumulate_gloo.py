"""compressed_reduce_scatter on CPU: two gloo ranks exchange compressed shards and sum them in float32.  The per-rank
codec here is the CPU oracle (test infrastructure): what is under test is the plumbing -- which shard goes where, the
trimmed exchange, the order of the sum."""
import os
import socket
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = 5008  # per shard


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _OracleAccumCodec:
    """CPU stand-in for GpuFloatCodec: compress, and decompress_accumulate = oracle decode, widen, numpy.float32 add."""

    def __init__(self, O):
        self.O = O

    def compress(self, tensors):
        O = self.O
        arch = [O.float_compress(O.BFLOAT16, t.contiguous().view(torch.int16).numpy().view(np.uint16), 10) for t in tensors]
        cap = max(O.float_max_compressed_size(O.BFLOAT16, t.numel()) for t in tensors)
        comp = torch.zeros((len(arch), cap), dtype=torch.uint8)
        for i, a in enumerate(arch):
            comp[i, : a.size] = torch.from_numpy(a.copy())
        return comp, torch.tensor([a.size for a in arch], dtype=torch.int32)

    def decompress_accumulate(self, rows, accs, accumulate):
        O = self.O
        status = torch.ones((len(rows),), dtype=torch.uint8)
        for i, (r, acc) in enumerate(zip(rows, accs)):
            rc, w, _ = O.float_decompress(O.BFLOAT16, r.numpy(), 10, acc.numel())
            assert rc == 0 and w.size == acc.numel()
            wide = (w.astype(np.uint32) << 16).view(np.float32)
            a = acc.numpy()
            a[:] = (a + wide).astype(np.float32) if accumulate else wide
        return status


def _tensor_of(rank, world):
    g = torch.Generator().manual_seed(300 + rank)
    return torch.randn(world * WORDS, generator=g).to(torch.bfloat16)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import oracle as O
    from dietgpu_amd import distributed as D

    D.init(backend="gloo")
    shard, stats = D.compressed_reduce_scatter(_tensor_of(rank, world), codec=_OracleAccumCodec(O))
    dist.barrier()
    q.put((rank, shard.numpy().view(np.uint32).copy(), stats))
    dist.destroy_process_group()


def test_compressed_reduce_scatter_world2():
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
    inputs = [_tensor_of(r, world).view(world, WORDS) for r in range(world)]
    for rank, bits, stats in res:
        # float32(shard of rank 0) + float32(shard of rank 1), straight from the inputs
        want = (inputs[0][rank].to(torch.float32).numpy() + inputs[1][rank].to(torch.float32).numpy()).astype(np.float32)
        assert bits.shape == (WORDS,)
        assert np.array_equal(bits, want.view(np.uint32)), f"rank {rank}: the reduced shard differs"
        assert stats["raw_bytes"] == world * WORDS * 2
        assert stats["wire_bytes"] < stats["raw_bytes"]  # bf16 N(0,1): fewer bytes on the wire than raw
        assert stats["payload_bytes"] < stats["raw_bytes"]
