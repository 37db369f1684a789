"""compressed_all_reduce(out=<16-bit parameters>, out_seed=) on CPU: two gloo ranks, the CPU oracle as the codec, in two
shapes -- one with a host `decompress_update` over tests/sr_ref.py, and one without the method, which takes the torch
fall-back (dietgpu_amd/rounding.py) -- on bfloat16 and float16 tensors, with and without clip_norm, out_scale and
out_accumulate.  Under test is the plumbing: the parameters have the same bits on both ranks and on both paths, equal to
sr_ref with source rank r as the member and the index within the shard as the word index; the calls are logged."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_accum_scaled_gloo import OUT_SCALE, _Codec, _archive_words, _bits32, _ft, _input, _np16
from test_accumulate_gloo import ROOT, WORDS, _free_port

KINDS = ("bf16", "fp16")
CODECS = ("update", "fallback")
SEED = 0x0123456789ABCDEF


class _FallbackCodec(_Codec):
    """decompress_accumulate without `scale`, no decompress_update"""

    def decompress_accumulate(self, *args, **kwargs):
        self.log.append(("decompress_accumulate", len(args), tuple(sorted(kwargs))))
        assert not kwargs
        rows, accs, accumulate = args
        return self._accumulate(rows, accs, accumulate, None)


class _UpdateCodec(_FallbackCodec):
    def decompress_update(self, rows, outs, accumulate, scale=None, seed=0, first_member=0):
        import sr_ref as S

        self.log.append(("decompress_update", bool(accumulate), scale is not None, first_member))
        if isinstance(seed, torch.Tensor):
            seed = int(seed.item()) & (2**64 - 1)
        for i, (r, out) in enumerate(zip(rows, outs)):
            w = self._words(r, out.numel())
            f = np.float32(1.0) if scale is None else np.float32(float(scale))
            got = S.update_ref(w, self.ft, f, seed, first_member + i, _np16(out) if accumulate else None)
            out.view(torch.int16).copy_(torch.from_numpy(got.view(np.int16).copy()))
        return torch.ones((len(rows),), dtype=torch.uint8)


_CODEC = {"update": _UpdateCodec, "fallback": _FallbackCodec}
#   case -> (keywords, the seed as a tensor)
CASES = {
    "store": ({}, False),
    "add": ({"out_accumulate": True}, True),
    "scaled add": ({"out_scale": OUT_SCALE, "out_accumulate": True}, False),
    "clipped store": ({"clip_norm": None}, False),
    "sgd": ({"out_scale": OUT_SCALE, "clip_norm": None, "out_accumulate": True}, True),
}


def _params(kind, world):
    g = torch.Generator().manual_seed(55)
    return (torch.randn(world * WORDS, generator=g) * 2.0).to(torch.bfloat16 if kind == "bf16" else torch.float16)


def _worker(rank, world, port, q, clips):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import oracle as O
    from dietgpu_amd import distributed as D

    D.init(backend="gloo")
    res = {}
    for kind in KINDS:
        x = _input(kind, rank, world)
        for name in CODECS:
            log = []
            codec = _CODEC[name](O, log)
            for case, (kwargs, seed_tensor) in CASES.items():
                kwargs = {k: (clips[kind] if k == "clip_norm" else v) for k, v in kwargs.items()}
                del log[:]
                buf = _params(kind, world)
                seed = torch.tensor([SEED], dtype=torch.int64) if seed_tensor else SEED
                out, stats = D.compressed_all_reduce(x.clone(), codec=codec, out=buf, out_seed=seed, **kwargs)
                assert out is buf
                coef = stats.get("clip_coef")
                res[kind, name, case] = (_np16(buf), list(log), None if coef is None else float(coef))
    dist.barrier()
    q.put((rank, res))
    dist.destroy_process_group()


def test_sixteen_bit_out_world2():
    import cast_ref as R
    import sr_ref as S

    world = 2
    words, clips = {}, {}
    for kind in KINDS:
        w, ft = _archive_words(kind, world)
        norm = float(np.sqrt(np.square(R.widen(w, ft).view(np.float32).astype(np.float64)).sum()))
        words[kind], clips[kind] = (w, ft), 0.5 * norm

    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, clips)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    f32 = np.float32
    for kind in KINDS:
        w, ft = words[kind]
        pre = _np16(_params(kind, world))
        for case, (kwargs, _) in CASES.items():
            coef = results[0][kind, "update", case][2]
            assert (coef is not None) == ("clip_norm" in kwargs), (kind, case)
            factor = f32(1.0)
            if "clip_norm" in kwargs:
                assert 0.49 < coef < 0.51
                factor = f32(coef)
            if "out_scale" in kwargs:
                factor = f32(OUT_SCALE) if "clip_norm" not in kwargs else f32(f32(coef) * f32(OUT_SCALE))  # one float32 multiply
            accumulate = bool(kwargs.get("out_accumulate"))
            want = np.concatenate([
                S.update_ref(w[r * WORDS:(r + 1) * WORDS], ft, factor, SEED, r, pre[r * WORDS:(r + 1) * WORDS] if accumulate else None)
                for r in range(world)])
            for rank in range(world):
                for name in CODECS:
                    got, log, got_coef = results[rank][kind, name, case]
                    what = f"{kind}, {case}, rank {rank}, {name} codec"
                    assert got_coef == coef, what
                    assert np.array_equal(got, want), f"{what}: differs from sr_ref"
                    tail = log[max(i for i, e in enumerate(log) if e[0] == "compress_cast") + 1:]
                    scaled = "clip_norm" in kwargs or "out_scale" in kwargs
                    if name == "update":
                        assert tail == [("decompress_update", accumulate, scaled, r) for r in range(world)], (what, tail)
                    else:
                        assert tail == [("decompress_accumulate", 3, ())] * world, (what, tail)
                    assert not any(e[0] == "decompress" for e in log), (what, log)
            if accumulate:  # the update moved the parameters, and by less than rounding to nearest would drop
                assert not np.array_equal(want, pre), (kind, case)


def test_argument_errors():
    from dietgpu_amd import distributed as D

    bf = torch.zeros(16, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="out_seed needs `out`"):
        D.compressed_all_reduce(bf, codec=object(), out_seed=1)
    with pytest.raises(RuntimeError, match="needs out_seed"):
        D.compressed_all_reduce(bf, codec=object(), out=torch.zeros(16, dtype=torch.bfloat16))
    for bad in (torch.zeros(16), torch.zeros(16, dtype=torch.float16), torch.zeros(15, dtype=torch.bfloat16),
                torch.zeros(4, 4, dtype=torch.bfloat16), torch.zeros(32, dtype=torch.bfloat16)[::2], "out"):
        with pytest.raises(RuntimeError, match="wire's 16-bit dtype"):
            D.compressed_all_reduce(bf, codec=object(), out=bad, out_seed=1)
    with pytest.raises(RuntimeError, match="wire's 16-bit dtype"):  # the wire's dtype, not the tensor's
        D.compressed_all_reduce(torch.zeros(16), codec=object(), wire_dtype=torch.float16, out=torch.zeros(16, dtype=torch.bfloat16), out_seed=1)
    ok = torch.zeros(16, dtype=torch.bfloat16)
    for bad in (-1, 2**64, 1.5, True, torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="out_seed must be|tensor out_seed"):
            D.compressed_all_reduce(bf, codec=object(), out=ok, out_seed=bad)
    with pytest.raises(RuntimeError, match="out_accumulate"):
        D.compressed_all_reduce(bf, codec=object(), out=bf, out_seed=1, out_accumulate=True)
