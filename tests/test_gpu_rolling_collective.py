"""The compressed collectives with GpuFloatCodec(rolling=True) at world 1 on RCCL: three runs on changing tensors deliver
bit for bit what rolling=False delivers (any table is lossless), and from the second run on no histogram kernel runs."""
import ctypes as C
import json
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _profiled(L, fn):
    L.dgpu_prof_reset()
    L.dgpu_prof_enable(1)
    try:
        result = fn()
        torch.cuda.synchronize()
    finally:
        L.dgpu_prof_enable(0)
    buf = C.create_string_buffer(8192)
    n = L.dgpu_prof_summary(buf, 8192)
    L.dgpu_prof_reset()
    return result, (json.loads(buf.value.decode()) if n > 0 else {})


def _counts_something(prof):
    return [k for k in prof if k.startswith("k_float_histogram") or k.startswith("k_histogram") or k == "k_stats_single"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rolling_codec_in_all_gather_and_all_reduce(dtype):
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    L = dietgpu_amd.lib()
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    D.init(backend="nccl", device=dev)  # "nccl" is RCCL on ROCm
    try:
        g = torch.Generator(device="cpu").manual_seed(23)
        plain, rolling = D.GpuFloatCodec(), D.GpuFloatCodec(rolling=True)
        assert rolling.rolling and not plain.rolling
        for run in range(3):
            scale = 1.0 + 0.7 * run
            ts = [(torch.randn(n, generator=g) * scale).to(dtype).to(dev) for n in (40_000 + 33, 9 * 4096, 500)]
            want, _ = D.compressed_all_gather(ts, codec=plain)
            (got, stats), prof = _profiled(L, lambda: D.compressed_all_gather(ts, codec=rolling))
            for a, b, t in zip(got[0], want[0], ts):
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(a.view(torch.int16), t.view(torch.int16))
            assert stats["payload_bytes"] < stats["raw_bytes"]
            assert bool(_counts_something(prof)) == (run == 0), (run, sorted(prof))

            x = (torch.randn(100_000 + 32, generator=g) * scale).to(dtype).to(dev)
            want, _ = D.compressed_all_reduce(x, codec=plain)
            (got, _), prof = _profiled(L, lambda: D.compressed_all_reduce(x, codec=rolling))
            assert torch.equal(got.view(torch.int16), want.view(torch.int16))
            assert bool(_counts_something(prof)) == (run == 0), (run, sorted(prof))
    finally:
        dist.destroy_process_group()
