"""compressed_all_reduce at world 1 on RCCL, with and without the one-call middle: the default codec sums the received
rows and writes the shard's archive in ONE reduce-compress call; the same codec with that method hidden takes the
three-step path (decode-reduce, cast-compress).  Both results are compared bit for bit with each other and with the input
-- the sum of one rank's tensor is the tensor, rounded once: cast_ref(widen(x)) = x."""
import os
import socket

import numpy as np
import pytest
import torch

import cast_ref as R

pytestmark = pytest.mark.gpu

WORDS = 8 * 4096 + 5  # per rank: 8 blocks and a partial one


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("dtype,ft", [(torch.bfloat16, R.BFLOAT16), (torch.float16, R.FLOAT16)])
def test_all_reduce_is_the_same_with_and_without_the_one_call_middle(dtype, ft):
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    dietgpu_amd.lib()
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    D.init(backend="nccl", device=dev)  # "nccl" is RCCL on ROCm
    try:
        g = torch.Generator(device="cpu").manual_seed(23)
        mine = torch.randn(WORDS, generator=g).to(dtype)
        words = mine.view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(R.cast_ref(R.widen(words, ft), ft), words)
        x = mine.to(dev)

        fused = D.GpuFloatCodec()
        calls = []
        inner = fused.decompress_reduce_compress

        def spy(rows_per_acc, accs, accumulate):
            calls.append(([len(r) for r in rows_per_acc], len(accs), accumulate))
            return inner(rows_per_acc, accs, accumulate)

        fused.decompress_reduce_compress = spy
        fused.decompress_reduce = fused.compress_cast = None  # (the three-step path would fail on them)
        out_one, stats_one = D.compressed_all_reduce(x, codec=fused)
        assert calls == [([1], 1, False)]

        plain = D.GpuFloatCodec()
        plain.decompress_reduce_compress = None  # hidden: not callable
        out_three, stats_three = D.compressed_all_reduce(x, codec=plain)

        default, _ = D.compressed_all_reduce(x)
        got = [t.view(torch.int16).cpu().numpy().view(np.uint16) for t in (out_one, out_three, default)]
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
        assert np.array_equal(got[0], words)
        assert out_one.dtype == dtype and out_one.shape == mine.shape
        assert stats_one == stats_three
        assert torch.equal(x.view(torch.int16).cpu(), mine.view(torch.int16))  # the input is unchanged
    finally:
        dist.destroy_process_group()
