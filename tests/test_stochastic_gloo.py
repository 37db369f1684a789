"""compressed_reduce_scatter / compressed_all_reduce(wire_seed=) on CPU: two gloo ranks, the CPU oracle as the codec, in two
shapes -- one with a host `compress_cast_stochastic` over tests/stochastic_ref.py, and one without the method, which takes
the torch fall-back (dietgpu_amd/rounding.py into a 16-bit scratch, then `compress`) -- on a float32 tensor with a
bfloat16 and a float16 wire and on a bfloat16 tensor without wire_dtype.  Under test is the plumbing: the result has the
same bits on both ranks and with both codecs, equal to a host model built from the reference with the member numbering
of the docstrings (first rounding: source rank * world + destination; second: world * world + shard); the calls are
logged, and without wire_seed the log is what it was."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_accum_scaled_gloo import _PlainCodec, _bits32, _ft, _np16
from test_accumulate_gloo import ROOT, WORDS, _free_port

KINDS = ("f32 on bf16", "f32 on fp16", "bf16")
CODECS = ("stochastic", "fallback")
SEED = 0xFEDCBA9876543210
#   case -> (keywords of compressed_all_reduce, the seed as a tensor)
CASES = {"sum": ({}, False), "avg, tensor seed": ({"op": "avg"}, True)}


def _input(kind, rank, world):
    g = torch.Generator().manual_seed(1300 + 10 * KINDS.index(kind) + rank)
    x = torch.randn(world * WORDS, generator=g) * 0.37
    return x.to(torch.bfloat16) if kind == "bf16" else x


def _wire(kind):
    return {"f32 on bf16": torch.bfloat16, "f32 on fp16": torch.float16, "bf16": None}[kind]


class _StochasticCodec(_PlainCodec):
    def compress_cast_stochastic(self, tensors, dtype, seed, first_member=0):
        import stochastic_ref as SR

        self.log.append(("compress_cast_stochastic", len(tensors), first_member))
        if isinstance(seed, torch.Tensor):
            seed = int(seed.item()) & (2**64 - 1)
        assert all(t.dtype == torch.float32 for t in tensors)
        return self._compress([torch.from_numpy(SR.words(_bits32(t), _ft(dtype), seed, first_member + i).view(np.int16)).view(dtype)
                               for i, t in enumerate(tensors)])


_CODEC = {"stochastic": _StochasticCodec, "fallback": _PlainCodec}


def _seed_tensor():
    return torch.tensor([SEED - (1 << 64)], dtype=torch.int64)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import oracle as O
    from dietgpu_amd import distributed as D

    D.init(backend="gloo")
    res = {}
    for kind in KINDS:
        x = _input(kind, rank, world)
        base = {} if _wire(kind) is None else {"wire_dtype": _wire(kind)}
        for name in CODECS:
            log = []
            codec = _CODEC[name](O, log)
            for case, (kwargs, as_tensor) in CASES.items():
                del log[:]
                out, _ = D.compressed_all_reduce(x.clone(), codec=codec, wire_seed=_seed_tensor() if as_tensor else SEED, **base, **kwargs)
                res[kind, name, case] = (_np16(out), list(log))
            # without wire_seed: the calls of today
            del log[:]
            out, _ = D.compressed_all_reduce(x.clone(), codec=codec, **base)
            res[kind, name, "nearest"] = (_np16(out), list(log))
            if _wire(kind) is not None:
                del log[:]
                shard, _ = D.compressed_reduce_scatter(x.clone(), codec=codec, wire_seed=SEED, **base)
                res[kind, name, "reduce-scatter"] = (_bits32(shard), list(log))
    dist.barrier()
    q.put((rank, res))
    dist.destroy_process_group()


def _model(kind, world, factor):
    """-> (the float32 bits of every rank's shard of the sum after the first rounding, the words of the all-reduce)"""
    import cast_ref as R
    import stochastic_ref as SR

    wire = _wire(kind)
    ft = _ft(wire if wire is not None else torch.bfloat16)
    xs = [_input(kind, r, world) for r in range(world)]
    shards, words = [], []
    for j in range(world):
        acc = None
        for r in range(world):
            part = xs[r][j * WORDS:(j + 1) * WORDS]
            q = SR.words(_bits32(part), ft, SEED, r * world + j) if wire is not None else _np16(part)
            wide = R.widen(q, ft).view(np.float32)
            acc = wide.copy() if acc is None else (acc + wide).astype(np.float32)  # the sequential float32 sum in rank order
        if factor is not None:
            acc = (acc * np.float32(factor)).astype(np.float32)
        shards.append(acc.view(np.uint32).copy())
        words.append(SR.words(acc.view(np.uint32), ft, SEED, world * world + j))
    return shards, np.concatenate(words)


def test_stochastic_wire_world2():
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    acc, dec = ("decompress_accumulate", 3, ()), ("decompress", 2, ())
    for kind in KINDS:
        wire = _wire(kind)
        for case, (kwargs, _) in CASES.items():
            shards, want = _model(kind, world, 0.5 if kwargs.get("op") == "avg" else None)
            for rank in range(world):
                for name in CODECS:
                    got, log = results[rank][kind, name, case]
                    what = f"{kind}, {case}, rank {rank}, {name} codec"
                    assert np.array_equal(got, want), f"{what}: differs from the host model"
                    if name == "stochastic":
                        first = ("compress_cast_stochastic", world, rank * world) if wire is not None else ("compress", 1, ())
                        assert log == [first] + [acc] * world + [("compress_cast_stochastic", 1, world * world + rank)] + [dec] * world, (what, log)
                    else:  # the rounding is torch's: the codec compresses 16-bit scratch tensors, and never rounds
                        assert log == [("compress", 1, ())] + [acc] * world + [("compress", 1, ())] + [dec] * world, (what, log)
        # the rounding to nearest is another result, and its calls are what they were
        nearest = results[0][kind, "stochastic", "nearest"][0]
        assert not np.array_equal(nearest, _model(kind, world, None)[1]), kind
        for rank in range(world):
            for name in CODECS:
                got, log = results[rank][kind, name, "nearest"]
                assert np.array_equal(got, nearest), (kind, rank, name)
                first = ("compress_cast", 2, ()) if wire is not None else ("compress", 1, ())
                assert log == [first] + [acc] * world + [("compress_cast", 2, ())] + [dec] * world, (kind, rank, name, log)
        if wire is not None:
            shards, _ = _model(kind, world, None)
            for rank in range(world):
                for name in CODECS:
                    got, log = results[rank][kind, name, "reduce-scatter"]
                    assert np.array_equal(got, shards[rank]), f"{kind}: reduce-scatter, rank {rank}, {name} codec"
                    first = ("compress_cast_stochastic", world, rank * world) if name == "stochastic" else ("compress", 1, ())
                    assert log == [first] + [acc] * world, (kind, rank, name, log)


class _WithFeedback:
    def compress_cast_feedback(self, *args):
        raise AssertionError("not reached")


def test_argument_errors():
    from dietgpu_amd import distributed as D

    f32, bf = torch.zeros(16), torch.zeros(16, dtype=torch.bfloat16)
    for call in (D.compressed_reduce_scatter, D.compressed_all_reduce):
        for bad in (-1, 2**64, 1.5, True, "seed", torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)):
            with pytest.raises(RuntimeError, match="wire_seed must be|tensor wire_seed"):
                call(f32, codec=object(), wire_dtype=torch.bfloat16, wire_seed=bad)
        with pytest.raises(RuntimeError, match="alternatives"):
            call(f32, codec=_WithFeedback(), wire_dtype=torch.bfloat16, wire_seed=1, residual=torch.zeros(16))
        with pytest.raises(RuntimeError, match="norm=True or clip_norm"):
            call(f32, codec=object(), wire_dtype=torch.bfloat16, wire_seed=1, norm=True)
    with pytest.raises(RuntimeError, match="norm=True or clip_norm"):
        D.compressed_all_reduce(f32, codec=object(), wire_dtype=torch.float16, wire_seed=1, clip_norm=1.0)
    with pytest.raises(RuntimeError, match="norm=True or clip_norm"):
        D.compressed_all_reduce(bf, codec=object(), wire_seed=torch.zeros(1, dtype=torch.int64), clip_norm=1.0)
    # in the reduce-scatter nothing is rounded without wire_dtype
    with pytest.raises(RuntimeError, match="wire_seed needs wire_dtype"):
        D.compressed_reduce_scatter(bf, codec=object(), wire_seed=1)
    with pytest.raises(RuntimeError, match="wire_seed needs wire_dtype"):
        D.compressed_reduce_scatter(f32, codec=object(), wire_seed=1)
    # a float32 tensor still needs its wire, and the old rules hold beside the seed
    with pytest.raises(RuntimeError, match="give wire_dtype"):
        D.compressed_all_reduce(f32, codec=object(), wire_seed=1)
    with pytest.raises(RuntimeError, match="raw_local cannot be combined with wire_dtype"):
        D.compressed_all_reduce(f32, codec=object(), wire_dtype=torch.bfloat16, wire_seed=1, raw_local=True)
