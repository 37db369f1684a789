"""compressed_all_reduce of a float32 tensor on a 16-bit wire with error feedback, at world 1 on RCCL with GpuFloatCodec:
two steps with one residual.  The sum of one rank's tensor is what that rank sent -- q of tests/feedback_ref.py, widened
and rounded once more, which changes nothing -- and the residual is the reference's after every step."""
import os
import socket

import numpy as np
import pytest
import torch

import feedback_ref as F

pytestmark = pytest.mark.gpu

BLK = 4096


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("dtype,ft", [(torch.bfloat16, F.BFLOAT16), (torch.float16, F.FLOAT16)])
def test_two_steps_of_all_reduce_with_a_residual_single_rank_rccl(dtype, ft):
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    dietgpu_amd.lib()
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    D.init(backend="nccl", device=dev)  # "nccl" is RCCL on ROCm
    try:
        world = dist.get_world_size()
        n = world * (2 * BLK + 100)
        codec = D.GpuFloatCodec()
        residual = torch.full((n,), float("nan"), device=dev)
        e = None
        for step in range(2):
            g = torch.Generator(device="cpu").manual_seed(23 + step)
            mine = torch.randn(n, generator=g) * 4.0
            x = mine.to(dev)
            out, stats = D.compressed_all_reduce(x, codec=codec, wire_dtype=dtype, residual=residual, residual_fresh=step == 0)
            q, e, _ = F.feedback_ref(mine.numpy().view(np.uint32), e, ft)
            assert out.dtype == dtype and out.shape == mine.shape and out.device == x.device
            assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), q), f"step {step}: the sum"
            assert np.array_equal(residual.view(torch.int32).cpu().numpy().view(np.uint32), e), f"step {step}: the residual"
            assert torch.equal(x.cpu(), mine)  # the input is unchanged
            assert stats["payload_bytes"] <= stats["wire_bytes"] < stats["raw_bytes"]
        # without a residual: plain rounding of the same tensor
        out, _ = D.compressed_all_reduce(x, codec=codec, wire_dtype=dtype)
        assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), F.cast_ref(mine.numpy().view(np.uint32), ft))
    finally:
        dist.destroy_process_group()
