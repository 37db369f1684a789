"""compressed_all_reduce(out=<16-bit parameters>, out_seed=) at world 1 on RCCL with the default codec: the parameters
come out of the decode kernel of the final all-gather (GpuFloatCodec.decompress_update), against a wrapper codec that
hides the method, so that the collectives' fall-back -- decode into a float32 scratch, the add and the stochastic rounding
in torch (dietgpu_amd/rounding.py) -- runs.  Bit for bit between the two and against tests/sr_ref.py.  The sum of one
rank's tensor is the tensor."""
import os

import numpy as np
import pytest
import torch

import cast_ref as R
import sr_ref as S
from test_gpu_reduce_scaled_all_reduce import _free_port

pytestmark = pytest.mark.gpu

WORDS = 5 * 4096 + 123
OUT_SCALE = -0.0625 * 1.1
SEED = 2**64 - 3
KINDS = [("f32 on bf16", torch.float32, torch.bfloat16, R.BFLOAT16), ("bf16", torch.bfloat16, None, R.BFLOAT16),
         ("fp16", torch.float16, None, R.FLOAT16)]


@pytest.mark.parametrize("kind,dtype,wire,ft", KINDS)
def test_sixteen_bit_parameters_out_of_the_all_reduce(kind, dtype, wire, ft):
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    dietgpu_amd.lib()
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    D.init(backend="nccl", device=dev)  # "nccl" is RCCL on ROCm
    try:
        out_dtype = wire if wire is not None else dtype
        g = torch.Generator(device="cpu").manual_seed(47)
        mine = torch.randn(WORDS, generator=g).to(dtype)
        pre = (torch.randn(WORDS, generator=g) * 3.0).to(out_dtype)
        x = mine.to(dev)
        base = {} if wire is None else {"wire_dtype": wire}
        bits16 = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16).copy()
        w16 = R.cast_ref(mine.numpy().view(np.uint32), ft) if wire is not None else bits16(mine)
        pre16 = bits16(pre)
        norm = float(np.sqrt(float(np.square(R.widen(w16, ft).view(np.float32).astype(np.float64)).sum())))
        clip = 0.25 * norm

        class Hidden(D.GpuFloatCodec):
            """GpuFloatCodec without decompress_update"""

            decompress_update = None

        calls = []

        class Spied(D.GpuFloatCodec):
            def decompress_update(self, rows, outs, accumulate, scale=None, seed=0, first_member=0):
                calls.append((len(rows), accumulate, None if scale is None else (scale.is_cuda, scale.dtype, scale.dim()), first_member))
                return D.GpuFloatCodec.decompress_update(self, rows, outs, accumulate, scale=scale, seed=seed, first_member=first_member)

            def decompress(self, *a, **k):
                raise AssertionError("with `out` the gather decodes with decompress_update")

        _, stats = D.compressed_all_reduce(x, clip_norm=clip, **base)
        coef = np.float32(float(stats["clip_coef"]))
        assert 0.24 < float(coef) < 0.26
        scale = np.float32(OUT_SCALE)
        both = np.float32(coef * scale)
        seed_dev = torch.tensor([SEED - 2**64], dtype=torch.int64, device=dev)
        cases = [
            ("store", {}, 1.0, False, SEED),
            ("add", {"out_accumulate": True}, 1.0, False, seed_dev),
            ("sgd", {"out_scale": OUT_SCALE, "out_accumulate": True}, scale, True, SEED),
            ("clipped sgd", {"out_scale": torch.tensor(OUT_SCALE, dtype=torch.float32, device=dev), "clip_norm": clip, "out_accumulate": True},
             both, True, seed_dev),
            ("clipped store", {"clip_norm": clip}, coef, True, SEED),
        ]
        for case, kwargs, factor, has_factor, seed in cases:
            acc = bool(kwargs.get("out_accumulate"))
            want = S.update_ref(w16, ft, factor, SEED, 0, pre16 if acc else None)
            got = {}
            for name, codec in (("kernel", Spied()), ("fall-back", Hidden())):
                del calls[:]
                buf = pre.to(dev)
                out, st = D.compressed_all_reduce(x, codec=codec, out=buf, out_seed=seed, **base, **kwargs)
                assert out is buf and out.dtype == out_dtype
                got[name] = bits16(buf)
                what = f"{kind} case {case}, {name}"
                assert np.array_equal(got[name], want), f"{what}: differs from the reference"
                if name == "kernel":  # one call for the one source rank, the factor a 0-dim float32 device tensor
                    assert calls == [(1, acc, (True, torch.float32, 0) if has_factor else None, 0)], f"{what}: {calls}"
            assert np.array_equal(got["kernel"], got["fall-back"]), f"{kind} case {case}: the kernel and the fall-back differ"
        with pytest.raises(RuntimeError):
            D.compressed_all_reduce(x, out=pre.to(dev), **base)                              # a 16-bit out without out_seed
        with pytest.raises(RuntimeError):
            D.compressed_all_reduce(x, out=torch.zeros(WORDS, device=dev), out_seed=1, **base)  # out_seed with a float32 out
    finally:
        dist.destroy_process_group()
