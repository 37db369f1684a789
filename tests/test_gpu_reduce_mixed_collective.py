"""raw_local of compressed_reduce_scatter / compressed_all_reduce at world 1 on RCCL, with the real codec: the rank's
own shard -- at world 1 the whole tensor -- is summed uncompressed by the mixed kernels, and the result has the bits of
the default path.  At world 1 nothing is left to compress on the way in: the reduce-scatter makes no compress call."""
import os

import numpy as np
import pytest
import torch

import cast_ref as R
from test_gpu_all_reduce import _free_port

pytestmark = pytest.mark.gpu


class _Counting:
    """a GpuFloatCodec whose calls are counted by name"""

    def __init__(self, codec):
        self._codec, self.calls = codec, []

    def __getattr__(self, name):
        attr = getattr(self._codec, name)
        if not callable(attr):
            return attr

        def counted(*args, **kwargs):
            self.calls.append(name)
            return attr(*args, **kwargs)

        return counted


@pytest.mark.parametrize("dtype,ft", [(torch.bfloat16, R.BFLOAT16), (torch.float16, R.FLOAT16)])
def test_raw_local_single_rank_rccl(dtype, ft):
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
        mine = torch.randn(100_000 + 33, generator=g).to(dtype)
        words = mine.view(torch.int16).numpy().view(np.uint16)
        x = mine.to(dev)

        # reduce-scatter: the float32 widening of the tensor, by either path
        plain = _Counting(D.GpuFloatCodec())
        shard0, stats0 = D.compressed_reduce_scatter(x, codec=plain)
        assert plain.calls == ["compress", "decompress_reduce"]
        mixed = _Counting(D.GpuFloatCodec())
        shard1, stats1 = D.compressed_reduce_scatter(x, codec=mixed, raw_local=True)
        assert mixed.calls == ["decompress_reduce_mixed"]  # no compress call at all
        assert shard1.dtype == torch.float32 and shard1.shape == mine.shape
        assert np.array_equal(shard1.cpu().numpy().view(np.uint32), shard0.cpu().numpy().view(np.uint32))
        assert np.array_equal(shard1.cpu().numpy().view(np.uint32), R.widen(words, ft))
        assert stats1["payload_bytes"] == 0 and stats1["wire_bytes"] == 0 and stats0["payload_bytes"] > 0
        assert stats1["raw_bytes"] == stats0["raw_bytes"]

        # all-reduce: the tensor itself, rounded once
        plain = _Counting(D.GpuFloatCodec())
        out0, _ = D.compressed_all_reduce(x, codec=plain)
        assert plain.calls == ["compress", "decompress_reduce_compress", "decompress"]
        mixed = _Counting(D.GpuFloatCodec())
        out1, _ = D.compressed_all_reduce(x, codec=mixed, raw_local=True)
        assert mixed.calls == ["decompress_reduce_compress_mixed", "decompress"]
        assert out1.dtype == dtype and out1.shape == mine.shape
        assert np.array_equal(out1.view(torch.int16).cpu().numpy().view(np.uint16), out0.view(torch.int16).cpu().numpy().view(np.uint16))
        assert np.array_equal(out1.view(torch.int16).cpu().numpy().view(np.uint16), words)
        assert torch.equal(x.view(torch.int16).cpu(), mine.view(torch.int16))  # the input is unchanged
    finally:
        dist.destroy_process_group()
