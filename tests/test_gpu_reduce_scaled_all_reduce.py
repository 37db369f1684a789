"""op="avg" and scale= of compressed_all_reduce at world 1 on RCCL with the default codec: the factor reaches the reduce
kernel on the one-call path (reduce-compress), on the three-step path (decode-reduce, then cast-compress; the one-call
method hidden) and with raw_local=True (the rank's own shard enters uncompressed).  The sum of one rank's tensor is the
tensor, so the result is cast_ref(widen(x) * f32(scale)) -- one float32 multiply, rounded once to the input dtype -- and
op="avg" at world 1 returns the input bits."""
import os
import socket

import numpy as np
import pytest
import torch

import cast_ref as R

pytestmark = pytest.mark.gpu

WORDS = 8 * 4096 + 5  # 8 blocks and a partial one
THIRD = 1.0 / 3.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("dtype,ft", [(torch.bfloat16, R.BFLOAT16), (torch.float16, R.FLOAT16)])
def test_scale_reaches_the_kernel_on_every_path(dtype, ft):
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    dietgpu_amd.lib()
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    D.init(backend="nccl", device=dev)  # "nccl" is RCCL on ROCm
    try:
        g = torch.Generator(device="cpu").manual_seed(29)
        mine = torch.randn(WORDS, generator=g).to(dtype)
        words = mine.view(torch.int16).numpy().view(np.uint16)
        x = mine.to(dev)
        wide = R.widen(words, ft).view(np.float32)
        want = R.cast_ref((wide * np.float32(THIRD)).astype(np.float32).view(np.uint32), ft)
        assert not np.array_equal(want, words)

        def bits(t):
            assert t.dtype == dtype and t.shape == mine.shape
            return t.view(torch.int16).cpu().numpy().view(np.uint16)

        # op="avg" in a world of one: a factor of 1, the input bits, and nothing new asked of the codec
        spied = D.GpuFloatCodec()
        calls = []
        inner = spied.decompress_reduce_compress

        def spy(rows_per_acc, accs, accumulate, **kw):
            calls.append((len(rows_per_acc[0]), accumulate, kw))
            return inner(rows_per_acc, accs, accumulate, **kw)

        spied.decompress_reduce_compress = spy  # (no `scale` parameter: with a factor the three-step path would run)
        out, _ = D.compressed_all_reduce(x, codec=spied, op="avg")
        assert np.array_equal(bits(out), words) and calls == [(1, False, {})]

        # the one-call path: the codec's own method, which has the parameter
        fused = D.GpuFloatCodec()
        seen = []
        inner_fused = fused.decompress_reduce_compress

        def spy_fused(rows_per_acc, accs, accumulate, scale=None):
            seen.append(scale)
            return inner_fused(rows_per_acc, accs, accumulate, scale=scale)

        fused.decompress_reduce_compress = spy_fused
        fused.decompress_reduce = fused.compress_cast = None  # (the three-step path would fail on them)
        out_one, stats_one = D.compressed_all_reduce(x, codec=fused, scale=THIRD)
        assert seen == [float(np.float32(THIRD))]
        assert np.array_equal(bits(out_one), want), "one-call path"

        # the three-step path: the one-call method hidden
        plain = D.GpuFloatCodec()
        plain.decompress_reduce_compress = None
        out_three, stats_three = D.compressed_all_reduce(x, codec=plain, scale=THIRD)
        assert np.array_equal(bits(out_three), want), "three-step path"
        assert stats_one == stats_three

        # raw_local: the own shard uncompressed, on both paths
        out_raw, _ = D.compressed_all_reduce(x, raw_local=True, scale=THIRD)
        assert np.array_equal(bits(out_raw), want), "raw_local, one-call path"
        out_raw3, _ = D.compressed_all_reduce(x, codec=plain, raw_local=True, scale=THIRD)
        assert np.array_equal(bits(out_raw3), want), "raw_local, three-step path"

        # the float32 shard of the reduce-scatter
        shard, _ = D.compressed_reduce_scatter(x, scale=THIRD)
        assert np.array_equal(shard.cpu().numpy().view(np.uint32), (wide * np.float32(THIRD)).astype(np.float32).view(np.uint32))

        default, _ = D.compressed_all_reduce(x, scale=THIRD)
        assert np.array_equal(bits(default), want)
        assert torch.equal(x.view(torch.int16).cpu(), mine.view(torch.int16))  # the input is unchanged
    finally:
        dist.destroy_process_group()
