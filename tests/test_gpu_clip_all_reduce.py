"""compressed_all_reduce(clip_norm=...) with the default codec: two ranks on one device (backend gloo, as the other
all-reduce tests on the GPU start them).  The clipped tensor is bit-identical on both ranks and equals
tests/scaled_ref.py of the unclipped sum at the coefficient computed here from that sum; the decode of the gather was
ops.decompress_data_scaled -- counted through a wrapper -- with the coefficient as a device tensor."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import cast_ref as R
import scaled_ref as S
from test_gpu_reduce_scaled_all_reduce import WORDS, _free_port

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP_FRACTION = 0.25  # clip_norm as a fraction of the norm of the sum


def _input(rank, dtype):
    g = torch.Generator(device="cpu").manual_seed(71 + rank)
    return torch.randn(2 * WORDS, generator=g).to(dtype)


def _worker(rank, world, port, q, dtype, clip_low, clip_high):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D
    from dietgpu_amd import ops

    dietgpu_amd.lib()
    dev = torch.device("cuda:0")  # both ranks on the one device
    torch.cuda.set_device(dev)
    D.init(backend="gloo")
    try:
        calls = []
        inner = ops.decompress_data_scaled

        def counted(ts_in, ts_out, scale, *a, **k):
            calls.append((len(ts_in), torch.is_tensor(scale) and scale.is_cuda and scale.dtype == torch.float32 and scale.numel() == 1))
            return inner(ts_in, ts_out, scale, *a, **k)

        ops.decompress_data_scaled = counted
        x = _input(rank, dtype).to(dev)
        words = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16).copy()
        res = {}
        out, stats = D.compressed_all_reduce(x)
        res["none"] = (words(out), None, len(calls), sorted(stats))
        for name, kw in (("low", {"clip_norm": clip_low}), ("high", {"clip_norm": clip_high}), ("low raw_local", {"clip_norm": clip_low, "raw_local": True}),
                         ("low avg", {"clip_norm": 0.5 * clip_low, "op": "avg"})):
            del calls[:]
            out, stats = D.compressed_all_reduce(x, **kw)
            torch.cuda.synchronize()
            coef = stats["clip_coef"]
            assert coef.dim() == 0 and coef.is_cuda and coef.dtype == torch.float32
            res[name] = (words(out), float(coef), list(calls), float(stats["global_sumsq"]), int(stats["global_nonfinite"]))
        dist.barrier()
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dtype,ft", [(torch.bfloat16, R.BFLOAT16), (torch.float16, R.FLOAT16)])
def test_clipped_all_reduce_two_ranks_on_one_device(dtype, ft):
    world = 2
    wide = [_input(r, dtype).to(torch.float32).numpy() for r in range(world)]
    total = (wide[0] + wide[1]).astype(np.float32)  # the float32 sum in rank order
    unclipped = R.cast_ref(total.view(np.uint32), ft)
    vals = R.widen(unclipped, ft).view(np.float32).astype(np.float64)
    sumsq = sum(float(np.square(vals[r * WORDS:(r + 1) * WORDS]).sum()) for r in range(world))
    norm = float(np.sqrt(sumsq))
    clip_low, clip_high = CLIP_FRACTION * norm, 4.0 * norm
    coef = np.float32(min(clip_low / (norm + 1e-6), 1.0))
    # (the mean: half the sum, clipped to half the bound -- the same coefficient up to the 1e-6 in the formula)
    mean = R.cast_ref((total * np.float32(0.5)).astype(np.float32).view(np.uint32), ft)
    mvals = R.widen(mean, ft).view(np.float32).astype(np.float64)
    mnorm = float(np.sqrt(sum(float(np.square(mvals[r * WORDS:(r + 1) * WORDS]).sum()) for r in range(world))))
    mcoef = np.float32(min(0.5 * clip_low / (mnorm + 1e-6), 1.0))

    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, dtype, clip_low, clip_high)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank in range(world):
        r = res[rank]
        what = f"{dtype} rank {rank}"
        assert np.array_equal(r["none"][0], unclipped), what
        assert r["none"][2] == 0 and "clip_coef" not in r["none"][3], f"{what}: without clip_norm nothing is scaled"
        for name, want_words, want_coef in (("low", S.scaled_ref(unclipped, ft, coef), coef), ("high", unclipped, np.float32(1.0)),
                                            ("low raw_local", S.scaled_ref(unclipped, ft, coef), coef), ("low avg", S.scaled_ref(mean, ft, mcoef), mcoef)):
            got, got_coef, calls, gsumsq, gnonfinite = r[name]
            print(what, name, "clip_coef", got_coef, "reference", float(want_coef), "global_sumsq", gsumsq)
            assert got_coef == float(want_coef), f"{what} {name}: clip_coef {got_coef!r}, the reference {float(want_coef)!r}"
            assert np.array_equal(got, want_words), f"{what} {name}: the tensor differs from the reference"
            assert gnonfinite == 0
            # the decode of the gather: one scaled call per rank's rows, the factor a 1-element float32 device tensor
            assert calls == [(1, True)] * world, f"{what} {name}: {calls}"
    for name in ("low", "high", "low raw_local", "low avg"):
        assert np.array_equal(res[0][name][0], res[1][name][0]), f"{dtype} {name}: the ranks differ"
