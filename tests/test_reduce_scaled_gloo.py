"""op="avg" and scale= of compressed_all_reduce / compressed_reduce_scatter on CPU: two gloo ranks, the CPU oracle as the
per-rank codec (test infrastructure).  What is under test is the plumbing: a codec whose methods have a `scale`
parameter is handed the factor (the one-call middle once, with the scale; or decompress_reduce on the three-step path),
a codec without one is called as it always was and the float32 shard is multiplied afterwards -- and every path gives
cast_ref(fl32((x0 + x1) * f)), the same bits on both ranks.  Default arguments call the codec with exactly three
positional arguments and no keyword."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_accumulate_gloo import ROOT, WORDS, _free_port, _tensor_of

THIRD = 1.0 / 3.0
KINDS = ("fused with scale", "reduce with scale", "no scale anywhere")


def _worker(rank, world, port, q, kind):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import oracle as O
    from dietgpu_amd import distributed as D
    from test_all_reduce_gloo import _OracleAllReduceCodec

    UNSET = "no keyword"

    class Logging(_OracleAllReduceCodec):
        def __init__(self, O):
            super().__init__(O)
            self.log = []

        def compress_cast(self, tensors, dtype):
            self.log.append(("cast",))
            return super().compress_cast(tensors, dtype)

        def _sum(self, rows_per_acc, accs, accumulate, scale):
            for rows, acc in zip(rows_per_acc, accs):
                for k, r in enumerate(rows):
                    _OracleAllReduceCodec.decompress_accumulate(self, [r], [acc], accumulate or k > 0)
                if scale is not UNSET and scale is not None:
                    a = acc.numpy()
                    a[:] = (a * np.float32(scale)).astype(np.float32)
            return torch.ones((len(accs),), dtype=torch.uint8)

    class ReduceWithScale(Logging):
        def decompress_reduce(self, rows_per_acc, accs, accumulate, scale=UNSET):
            self.log.append(("reduce", [len(r) for r in rows_per_acc], bool(accumulate), scale))
            return self._sum(rows_per_acc, accs, accumulate, scale)

    class FusedWithScale(ReduceWithScale):
        def decompress_reduce_compress(self, rows_per_acc, accs, accumulate, scale=UNSET):
            self.log.append(("fused", [len(r) for r in rows_per_acc], bool(accumulate), scale))
            status = self._sum(rows_per_acc, accs, accumulate, scale)
            comp, sizes = _OracleAllReduceCodec.compress_cast(self, accs, torch.bfloat16)
            return status, comp, sizes

    class NoScale(Logging):
        def decompress_reduce(self, rows_per_acc, accs, accumulate):
            self.log.append(("reduce", [len(r) for r in rows_per_acc], bool(accumulate), UNSET))
            return self._sum(rows_per_acc, accs, accumulate, UNSET)

        def decompress_reduce_compress(self, rows_per_acc, accs, accumulate):
            self.log.append(("fused", [len(r) for r in rows_per_acc], bool(accumulate), UNSET))
            status = self._sum(rows_per_acc, accs, accumulate, UNSET)
            comp, sizes = _OracleAllReduceCodec.compress_cast(self, accs, torch.bfloat16)
            return status, comp, sizes

    D.init(backend="gloo")
    make = {KINDS[0]: FusedWithScale, KINDS[1]: ReduceWithScale, KINDS[2]: NoScale}[kind]
    x = _tensor_of(rank, world)
    before = x.clone()
    results = {}
    for name, kw in (("avg", {"op": "avg"}), ("third", {"scale": THIRD}), ("default", {}), ("avg times two", {"op": "avg", "scale": 2.0})):
        codec = make(O)
        out, _ = D.compressed_all_reduce(x, codec=codec, **kw)
        results[name] = (out.view(torch.int16).numpy().view(np.uint16).copy(), codec.log)
    codec = make(O)
    shard, _ = D.compressed_reduce_scatter(x, codec=codec, op="avg")
    results["scatter"] = (shard.numpy().view(np.uint32).copy(), codec.log)
    failures = []
    for bad in ({"op": "max"}, {"scale": 0.0}, {"scale": float("inf")}, {"op": "avg", "scale": float("nan")}):
        try:
            D.compressed_all_reduce(x, codec=make(O), **bad)
            failures.append(bad)
        except (ValueError, RuntimeError):
            pass
    dist.barrier()
    assert torch.equal(x.view(torch.int16), before.view(torch.int16))
    q.put((rank, results, failures))
    dist.destroy_process_group()


@pytest.mark.parametrize("kind", KINDS)
def test_avg_and_scale_on_every_codec_path(kind):
    import cast_ref as R

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
    inputs = [_tensor_of(r, world) for r in range(world)]
    total = (inputs[0].to(torch.float32).numpy() + inputs[1].to(torch.float32).numpy()).astype(np.float32)

    def times(f):
        return (total * np.float32(f)).astype(np.float32)

    half, third = float(np.float32(0.5)), float(np.float32(THIRD))
    UNSET = "no keyword"
    for rank, results, failures in res:
        assert failures == [], f"rank {rank}: accepted {failures}"
        for name, f in (("avg", 0.5), ("third", THIRD), ("default", 1.0), ("avg times two", 1.0)):
            assert np.array_equal(results[name][0], R.cast_ref(times(f).view(np.uint32), R.BFLOAT16)), f"rank {rank}, {kind}: {name}"
        assert np.array_equal(results["scatter"][0], times(0.5).view(np.uint32)[rank * WORDS : (rank + 1) * WORDS]), f"rank {rank}, {kind}: scatter"
        logs = {name: log for name, (_, log) in results.items()}
        if kind == KINDS[0]:  # one fused call, once, with the scale passed
            assert logs["avg"] == [("fused", [world], False, half)]
            assert logs["third"] == [("fused", [world], False, third)]
            assert logs["scatter"] == [("reduce", [world], False, half)]
        elif kind == KINDS[1]:  # the three-step path, the scale in its reduce call
            assert logs["avg"] == [("reduce", [world], False, half), ("cast",)]
            assert logs["third"] == [("reduce", [world], False, third), ("cast",)]
            assert logs["scatter"] == [("reduce", [world], False, half)]
        else:  # nothing new is asked of the codec: the shard is multiplied after the sum
            assert logs["avg"] == logs["third"] == [("reduce", [world], False, UNSET), ("cast",)]
            assert logs["scatter"] == [("reduce", [world], False, UNSET)]
        # default arguments, and a factor of exactly 1: three positional arguments and no keyword
        want_default = [("reduce", [world], False, UNSET), ("cast",)] if kind == KINDS[1] else [("fused", [world], False, UNSET)]
        assert logs["default"] == want_default and logs["avg times two"] == want_default
