"""compressed_all_reduce(wire_seed=) at world 1 on RCCL with the default codec: both roundings of the sending side come out
of the compressor's kernels (GpuFloatCodec.compress_cast_stochastic), against a wrapper codec that hides the method, so
that the collectives' fall-back -- dietgpu_amd/rounding.py into a 16-bit scratch, then `compress` -- runs.  Bit for bit
between the two and against tests/stochastic_ref.py: member 0 for the first rounding of the one rank's one shard, member
world * world + rank = 1 for the rounding of the sum.  The sum of one rank's tensor is the tensor."""
import os

import numpy as np
import pytest
import torch

import cast_ref as R
import stochastic_ref as SR
from test_gpu_reduce_scaled_all_reduce import _free_port

pytestmark = pytest.mark.gpu

WORDS = 5 * 4096 + 123
SEED = 2**64 - 3
KINDS = [("f32 on bf16", torch.float32, torch.bfloat16, R.BFLOAT16), ("f32 on fp16", torch.float32, torch.float16, R.FLOAT16),
         ("bf16", torch.bfloat16, None, R.BFLOAT16), ("fp16", torch.float16, None, R.FLOAT16)]


@pytest.mark.parametrize("kind,dtype,wire,ft", KINDS)
def test_stochastic_wire_of_the_all_reduce(kind, dtype, wire, ft):
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    dietgpu_amd.lib()
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    D.init(backend="nccl", device=dev)  # "nccl" is RCCL on ROCm
    try:
        g = torch.Generator(device="cpu").manual_seed(53)
        mine = (torch.randn(WORDS, generator=g) * 0.37).to(dtype)
        x = mine.to(dev)
        base = {} if wire is None else {"wire_dtype": wire}
        bits16 = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16).copy()
        # first rounding (member 0 * 1 + 0), the exact widening, second rounding (member 1 * 1 + 0)
        first = SR.words(mine.numpy().view(np.uint32), ft, SEED, 0) if wire is not None else bits16(mine)
        want = SR.words(R.widen(first, ft), ft, SEED, 1)
        if wire is None:
            assert np.array_equal(want, first)  # a representable value never moves

        class Hidden(D.GpuFloatCodec):
            """GpuFloatCodec without compress_cast_stochastic"""

            compress_cast_stochastic = None

        calls = []

        class Spied(D.GpuFloatCodec):
            def compress_cast_stochastic(self, tensors, dtype, seed, first_member=0):
                calls.append((len(tensors), dtype, first_member))
                return D.GpuFloatCodec.compress_cast_stochastic(self, tensors, dtype, seed, first_member=first_member)

            def compress_cast(self, *a, **k):
                raise AssertionError("with wire_seed nothing is rounded to nearest")

        seed_dev = torch.tensor([SEED - 2**64], dtype=torch.int64, device=dev)
        out_dtype = wire if wire is not None else dtype
        for seed in (SEED, seed_dev):
            got = {}
            for name, codec in (("kernel", Spied()), ("fall-back", Hidden())):
                del calls[:]
                out, _ = D.compressed_all_reduce(x, codec=codec, wire_seed=seed, **base)
                assert out.dtype == out_dtype
                got[name] = bits16(out)
                assert np.array_equal(got[name], want), f"{kind}, {name}: differs from the reference"
                if name == "kernel":
                    assert calls == ([(1, wire, 0)] if wire is not None else []) + [(1, out_dtype, 1)], calls
            assert np.array_equal(got["kernel"], got["fall-back"]), f"{kind}: the kernel and the fall-back differ"
        if wire is not None:
            shard, _ = D.compressed_reduce_scatter(x, wire_seed=SEED, **base)
            assert np.array_equal(shard.view(torch.int32).cpu().numpy().view(np.uint32), R.widen(first, ft)), f"{kind}: reduce-scatter"
            nearest, _ = D.compressed_all_reduce(x, **base)
            assert not np.array_equal(bits16(nearest), want)
        with pytest.raises(RuntimeError):
            D.compressed_all_reduce(x, wire_seed=SEED, norm=True, **base)
        assert int(seed_dev.item()) == SEED - 2**64, "the seed tensor was written"
    finally:
        dist.destroy_process_group()
