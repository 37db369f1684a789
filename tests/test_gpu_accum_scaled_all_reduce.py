"""compressed_all_reduce(out=, out_scale=, out_accumulate=) at world 1 on RCCL with the default codec: the float32 result
comes out of the decode kernel of the final all-gather (GpuFloatCodec.decompress_accumulate with its `scale`, on the
one-call path of the reduce), against a wrapper codec that hides the parameter, so that the collectives' fall-back --
decode-accumulate into a scratch, `mul_`, `copy_` / `add_` -- runs.  Bit for bit between the two, against
tests/accum_scaled_ref.py, and against today's 16-bit result.  The sum of one rank's tensor is the tensor."""
import os

import numpy as np
import pytest
import torch

import accum_scaled_ref as A
import cast_ref as R
from test_gpu_reduce_scaled_all_reduce import _free_port

pytestmark = pytest.mark.gpu

WORDS = 5 * 4096 + 123
OUT_SCALE = -0.0625 * 1.1
KINDS = [("f32 on bf16", torch.float32, torch.bfloat16, R.BFLOAT16), ("f32 on fp16", torch.float32, torch.float16, R.FLOAT16),
         ("bf16", torch.bfloat16, None, R.BFLOAT16), ("fp16", torch.float16, None, R.FLOAT16)]


@pytest.mark.parametrize("kind,dtype,wire,ft", KINDS)
def test_float32_out_of_the_all_reduce(kind, dtype, wire, ft):
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    dietgpu_amd.lib()
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    D.init(backend="nccl", device=dev)  # "nccl" is RCCL on ROCm
    try:
        g = torch.Generator(device="cpu").manual_seed(43)
        mine = torch.randn(WORDS, generator=g).to(dtype)
        pre = torch.randn(WORDS, generator=g) * 3.0
        x = mine.to(dev)
        base = {} if wire is None else {"wire_dtype": wire}
        w16 = R.cast_ref(mine.numpy().view(np.uint32), ft) if wire is not None else mine.view(torch.int16).numpy().view(np.uint16).copy()
        vals = R.widen(w16, ft).view(np.float32).astype(np.float64)
        norm = float(np.sqrt(float(np.square(vals).sum())))
        clip = 0.25 * norm

        class Hidden(D.GpuFloatCodec):
            """GpuFloatCodec whose decompress_accumulate has no `scale` parameter"""

            def decompress_accumulate(self, rows, accs, accumulate):
                return D.GpuFloatCodec.decompress_accumulate(self, rows, accs, accumulate)

        calls = []

        class Spied(D.GpuFloatCodec):
            def decompress_accumulate(self, rows, accs, accumulate, scale=None):
                calls.append((len(rows), accumulate, None if scale is None else (scale.is_cuda, scale.dtype, scale.dim())))
                return D.GpuFloatCodec.decompress_accumulate(self, rows, accs, accumulate, scale=scale)

            def decompress(self, *a, **k):
                raise AssertionError("with `out` the gather decodes with decompress_accumulate")

        bits32 = lambda t: t.cpu().numpy().view(np.uint32).copy()
        bits16 = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16).copy()
        today, _ = D.compressed_all_reduce(x, **base)
        assert np.array_equal(bits16(today), w16)
        today_clip, stats = D.compressed_all_reduce(x, clip_norm=clip, **base)
        coef = np.float32(float(stats["clip_coef"]))
        assert abs(float(coef) - min(clip / (norm + 1e-6), 1.0)) <= 1e-6 and 0.24 < float(coef) < 0.26
        scale = np.float32(OUT_SCALE)
        both = np.float32(coef * scale)
        pre_bits = pre.numpy().view(np.uint32)
        cases = [
            ("i", {}, R.widen(w16, ft), False),
            ("ii", {"clip_norm": clip}, A.accum_scaled_ref(w16, ft, coef), True),
            ("iii number", {"out_scale": OUT_SCALE}, A.accum_scaled_ref(w16, ft, scale), True),
            ("iii tensor", {"out_scale": torch.tensor([OUT_SCALE], dtype=torch.float32, device=dev)}, A.accum_scaled_ref(w16, ft, scale), True),
            ("iii number clip", {"out_scale": OUT_SCALE, "clip_norm": clip}, A.accum_scaled_ref(w16, ft, both), True),
            ("iii tensor clip", {"out_scale": torch.tensor(OUT_SCALE, dtype=torch.float32, device=dev), "clip_norm": clip},
             A.accum_scaled_ref(w16, ft, both), True),
            ("iv", {"out_scale": OUT_SCALE, "clip_norm": clip, "out_accumulate": True}, A.accum_scaled_ref(w16, ft, both, pre_bits), True),
            ("iv plain", {"out_accumulate": True}, A.accum_scaled_ref(w16, ft, 1.0, pre_bits), False),
        ]
        for case, kwargs, want, has_factor in cases:
            got = {}
            for name, codec in (("kernel", Spied()), ("fall-back", Hidden())):
                del calls[:]
                buf = pre.to(dev) if kwargs.get("out_accumulate") else torch.full((WORDS,), float("nan"), device=dev)
                out, st = D.compressed_all_reduce(x, codec=codec, out=buf, **base, **kwargs)
                assert out is buf and out.dtype == torch.float32
                got[name] = bits32(buf)
                what = f"{kind} case {case}, {name}"
                assert np.array_equal(got[name], want), f"{what}: differs from the reference"
                if "clip_norm" in kwargs:
                    assert np.float32(float(st["clip_coef"])) == coef, what
                if name == "kernel":  # one call for the one source rank, the factor a 0-dim float32 device tensor
                    acc = bool(kwargs.get("out_accumulate"))
                    assert calls == [(1, acc, (True, torch.float32, 0) if has_factor else None)], f"{what}: {calls}"
            assert np.array_equal(got["kernel"], got["fall-back"]), f"{kind} case {case}: the kernel and the fall-back differ"
            if case == "i":
                assert np.array_equal(got["kernel"], bits32(today.float())), "(i) is today's result .float()"
            if case == "ii":
                narrowed = torch.from_numpy(got["kernel"].view(np.float32).copy()).to(today.dtype)
                assert np.array_equal(bits16(narrowed), bits16(today_clip)), "(ii).to(dtype) has the bits of today's clipped result"
        if dtype == torch.float32:  # (v) out is tensor: an in-place float32 all-reduce on the 16-bit wire
            for name, codec in (("kernel", Spied()), ("fall-back", Hidden())):
                t = x.clone()
                out, _ = D.compressed_all_reduce(t, codec=codec, out=t, out_scale=OUT_SCALE, **base)
                assert out is t
                assert np.array_equal(bits32(t), A.accum_scaled_ref(w16, ft, scale)), f"{kind} case v, {name}"
            with pytest.raises(RuntimeError):
                D.compressed_all_reduce(x, out=x, out_accumulate=True, **base)
        assert torch.equal(x.cpu().view(torch.int32 if dtype == torch.float32 else torch.int16),
                           mine.view(torch.int32 if dtype == torch.float32 else torch.int16))  # the input is unchanged
    finally:
        dist.destroy_process_group()
