"""compressed_all_reduce at world 1 on RCCL: reduce-scatter into float32, cast-compress of the shard, compressed
all-gather -- the sum of one rank's tensor is the tensor, rounded once: cast_ref(widen(x)) = x, bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch

import cast_ref as R

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("dtype,ft", [(torch.bfloat16, R.BFLOAT16), (torch.float16, R.FLOAT16)])
def test_compressed_all_reduce_single_rank_rccl(dtype, ft):
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    dietgpu_amd.lib()
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    D.init(backend="nccl", device=dev)  # "nccl" is RCCL on ROCm
    try:
        g = torch.Generator(device="cpu").manual_seed(19)
        mine = torch.randn(100_000 + 33, generator=g).to(dtype)
        words = mine.view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(R.cast_ref(R.widen(words, ft), ft), words)
        x = mine.to(dev)
        out, stats = D.compressed_all_reduce(x)
        assert out.dtype == dtype and out.shape == mine.shape and out.device == x.device
        assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), words)
        assert torch.equal(x.view(torch.int16).cpu(), mine.view(torch.int16))  # the input is unchanged
        assert stats["raw_bytes"] == 2 * mine.numel() * 2
        assert stats["payload_bytes"] <= stats["wire_bytes"] < stats["raw_bytes"]  # N(0, 1): fewer bytes on the wire than raw
    finally:
        dist.destroy_process_group()
