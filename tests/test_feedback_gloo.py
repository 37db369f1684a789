"""float32 tensors on a bfloat16 wire with error feedback, on CPU: two gloo ranks run three steps of
compressed_reduce_scatter and of compressed_all_reduce with wire_dtype=bfloat16 and a residual.  The per-rank codec is the
CPU oracle of tests/test_all_reduce_gloo.py with a compress_cast_feedback built on tests/feedback_ref.py, and it logs its
calls: what is under test is the plumbing -- which call the shards go through, with which views of the residual, `fresh`
only where asked, and nothing new for the calls that were there before."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_accumulate_gloo import ROOT, WORDS, _free_port
from test_all_reduce_gloo import _OracleAllReduceCodec

STEPS = 3


class _LoggingFeedbackCodec(_OracleAllReduceCodec):
    def __init__(self, O):
        super().__init__(O)
        self.log = []

    def compress(self, tensors):
        self.log.append(("compress", len(tensors), str(tensors[0].dtype)))
        return super().compress(tensors)

    def _quiet_compress(self, tensors):
        return _OracleAllReduceCodec.compress(self, tensors)

    def compress_cast(self, tensors, dtype):
        import cast_ref as R

        self.log.append(("compress_cast", len(tensors), str(dtype)))
        rounded = [torch.from_numpy(R.cast_ref(t.contiguous().numpy().view(np.uint32), R.BFLOAT16).view(np.int16)).view(torch.bfloat16)
                   for t in tensors]
        return self._quiet_compress(rounded)

    def compress_cast_feedback(self, tensors, residuals, dtype, fresh=False):
        import feedback_ref as F

        assert dtype == torch.bfloat16
        self.log.append(("compress_cast_feedback", len(tensors), [r.data_ptr() for r in residuals], [r.numel() for r in residuals], fresh))
        rounded = []
        for t, r in zip(tensors, residuals):
            q, err, _ = F.feedback_ref(t.contiguous().numpy().view(np.uint32), None if fresh else r.numpy().view(np.uint32), F.BFLOAT16)
            r.view(torch.int32).copy_(torch.from_numpy(err.view(np.int32).copy()))
            rounded.append(torch.from_numpy(q.view(np.int16).copy()).view(torch.bfloat16))
        return self._quiet_compress(rounded)


class _NoFeedbackCodec(_OracleAllReduceCodec):
    compress_cast_feedback = None


def _tensor32(rank, step, world):
    g = torch.Generator().manual_seed(700 + 10 * step + rank)
    return torch.randn(world * WORDS, generator=g) * 3.0


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import oracle as O
    from dietgpu_amd import distributed as D

    D.init(backend="gloo")
    out = {"rank": rank}
    for name, call in (("reduce_scatter", D.compressed_reduce_scatter), ("all_reduce", D.compressed_all_reduce)):
        codec = _LoggingFeedbackCodec(O)
        residual = torch.full((world * WORDS,), float("nan"))
        views = [residual.data_ptr() + j * WORDS * 4 for j in range(world)]
        results, residuals = [], []
        for step in range(STEPS):
            x = _tensor32(rank, step, world)
            before = x.clone()
            got, _ = call(x, codec=codec, wire_dtype=torch.bfloat16, residual=residual, residual_fresh=step == 0)
            assert torch.equal(x, before)
            results.append((str(got.dtype), got.view(torch.int32 if got.dtype == torch.float32 else torch.int16).numpy().copy()))
            residuals.append(residual.numpy().view(np.uint32).copy())
        fb = [e for e in codec.log if e[0] == "compress_cast_feedback"]
        assert len(fb) == STEPS, codec.log
        for step, e in enumerate(fb):
            assert e[1:] == (world, views, [WORDS] * world, step == 0), e
        assert not [e for e in codec.log if e[0] == "compress"], codec.log
        # (the all-reduce rounds its shard of the sum with compress_cast, once per step; the reduce-scatter never)
        assert len([e for e in codec.log if e[0] == "compress_cast"]) == (STEPS if name == "all_reduce" else 0), codec.log
        out[name] = (results, residuals)
    # without a residual the shards go through compress_cast
    codec = _LoggingFeedbackCodec(O)
    shard, _ = D.compressed_reduce_scatter(_tensor32(rank, 0, world), codec=codec, wire_dtype=torch.bfloat16)
    assert [e[0] for e in codec.log] == ["compress_cast"] and codec.log[0][1:] == (world, "torch.bfloat16"), codec.log
    out["no_residual"] = shard.numpy().view(np.uint32).copy()
    # with the defaults and a bf16 tensor the call log is today's: one compress of the shards, one compress_cast of the sum
    codec = _LoggingFeedbackCodec(O)
    D.compressed_all_reduce(_tensor32(rank, 0, world).to(torch.bfloat16), codec=codec)
    assert codec.log == [("compress", world, "torch.bfloat16"), ("compress_cast", 1, "torch.bfloat16")], codec.log
    # the errors, on every rank, before anything is exchanged
    x = _tensor32(rank, 0, world)
    with pytest.raises(RuntimeError, match="raw_local"):
        D.compressed_all_reduce(x, codec=_LoggingFeedbackCodec(O), wire_dtype=torch.bfloat16, raw_local=True)
    with pytest.raises(RuntimeError, match="compress_cast_feedback"):
        D.compressed_reduce_scatter(x, codec=_NoFeedbackCodec(O), wire_dtype=torch.bfloat16, residual=torch.zeros_like(x))
    dist.barrier()
    q.put(out)
    dist.destroy_process_group()


def test_three_steps_with_a_residual_world2():
    import cast_ref as R
    import feedback_ref as F

    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in range(world)), key=lambda o: o["rank"])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # the reference: per rank, three feedback steps over the whole tensor (the shards are its contiguous parts)
    e = [None] * world
    for step in range(STEPS):
        wide = []
        for r in range(world):
            qw, e[r], _ = F.feedback_ref(_tensor32(r, step, world).numpy().view(np.uint32), e[r], F.BFLOAT16)
            wide.append(R.widen(qw, R.BFLOAT16).view(np.float32))
        total = (wide[0] + wide[1]).astype(np.float32)  # the rank-ordered float32 sum of the widened rows
        for r in range(world):
            for name in ("reduce_scatter", "all_reduce"):
                results, residuals = res[r][name]
                assert np.array_equal(residuals[step], e[r]), f"rank {r} {name} step {step}: the residual differs"
            dtype, got = res[r]["reduce_scatter"][0][step]
            assert dtype == "torch.float32"
            assert np.array_equal(got.view(np.uint32), total.view(np.uint32)[r * WORDS : (r + 1) * WORDS]), f"rank {r} step {step}: shard"
            dtype, got = res[r]["all_reduce"][0][step]
            assert dtype == "torch.bfloat16"  # the sum comes back in the wire dtype, rounded once more (no feedback there)
            assert np.array_equal(got.view(np.uint16), R.cast_ref(total.view(np.uint32), R.BFLOAT16)), f"rank {r} step {step}: all-reduce"
        if step == 0:
            for r in range(world):  # no residual: plain rounding, which is what a fresh step sends too
                assert np.array_equal(res[r]["no_residual"], total.view(np.uint32)[r * WORDS : (r + 1) * WORDS])
