"""compressed_all_reduce(clip_norm=...) and compressed_all_gather(scale=...) on CPU: two gloo ranks, the CPU oracle as
the codec (tests/test_all_reduce_gloo.py), once with a `decompress` that takes a `scale` -- it applies tests/scaled_ref.py
-- and once without, which the collectives then scale with one pass of torch.  Under test is the plumbing: the
statistics are all-reduced BEFORE the gather, the coefficient is clip_grad_norm_'s, it reaches the decode, and without
clip_norm every codec call is the one it always was."""
import os
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

from test_accumulate_gloo import ROOT, WORDS, _free_port, _tensor_of
from test_all_reduce_gloo import _OracleAllReduceCodec

GATHER_SCALE = 1.0 / 3.0


class _Logged:
    """the codec calls and the all-reduces of one collective, in order"""

    def __init__(self):
        self.log = []


class _PlainCodec(_OracleAllReduceCodec):
    """decompress(rows, outs): no `scale` parameter"""

    def __init__(self, O, logged):
        super().__init__(O)
        self.logged = logged

    def compress(self, tensors):
        self.logged.log.append(("compress", 1, ()))
        return super().compress(tensors)

    def compress_cast(self, tensors, dtype):
        self.logged.log.append(("compress_cast", 2, ()))
        return _OracleAllReduceCodec.compress(self, [self._rounded(t) for t in tensors])

    @staticmethod
    def _rounded(t):
        import cast_ref as R

        return torch.from_numpy(R.cast_ref(t.contiguous().numpy().view(np.uint32), R.BFLOAT16).view(np.int16)).view(torch.bfloat16)

    def decompress_accumulate(self, *args, **kwargs):
        self.logged.log.append(("decompress_accumulate", len(args), tuple(sorted(kwargs))))
        return super().decompress_accumulate(*args, **kwargs)

    def decompress(self, *args, **kwargs):
        self.logged.log.append(("decompress", len(args), tuple(sorted(kwargs))))
        rows, outs = args
        assert not kwargs
        return _OracleAllReduceCodec.decompress(self, rows, outs)


class _ScalingCodec(_PlainCodec):
    def decompress(self, rows, outs, scale=None):
        import scaled_ref as S

        self.logged.log.append(("decompress", 2, () if scale is None else ("scale",)))
        status = _OracleAllReduceCodec.decompress(self, rows, outs)
        if scale is not None:
            f = np.float32(float(scale))
            for o in outs:
                w = o.view(torch.int16).numpy().view(np.uint16)
                o.view(torch.int16).copy_(torch.from_numpy(S.scaled_ref(w, S.BFLOAT16, f).view(np.int16).copy()))
        return status


def _words(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def _worker(rank, world, port, q, clip_low, clip_high):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import oracle as O
    from dietgpu_amd import distributed as D

    D.init(backend="gloo")
    logged = _Logged()
    real_all_reduce = dist.all_reduce

    def all_reduce(t, *a, **k):
        logged.log.append(("all_reduce", str(t.dtype), tuple(t.shape)))
        return real_all_reduce(t, *a, **k)

    dist.all_reduce = all_reduce
    x = _tensor_of(rank, world)
    res = {}
    for kind, codec in (("scaling", _ScalingCodec(O, logged)), ("plain", _PlainCodec(O, logged))):
        for name, kwargs in (("none", {}), ("norm", {"norm": True}), ("low", {"clip_norm": clip_low}), ("high", {"clip_norm": clip_high})):
            logged.log = []
            out, stats = D.compressed_all_reduce(x.clone(), codec=codec, **kwargs)
            coef = stats.get("clip_coef")
            res[kind, name] = (_words(out), list(logged.log), None if coef is None else (str(coef.dtype), tuple(coef.shape), float(coef)),
                               float(stats["global_sumsq"]) if "global_sumsq" in stats else None, sorted(stats))
        logged.log = []
        mine = [x[:WORDS].clone(), x[WORDS:].clone()]
        gathered, _ = D.compressed_all_gather(mine, codec=codec, scale=GATHER_SCALE)
        res[kind, "gather"] = ([[_words(t) for t in per_rank] for per_rank in gathered], list(logged.log))
        logged.log = []
        gathered, _ = D.compressed_all_gather(mine, codec=codec, scale=torch.tensor(GATHER_SCALE, dtype=torch.float32))
        res[kind, "gather_tensor"] = ([[_words(t) for t in per_rank] for per_rank in gathered], list(logged.log))
        logged.log = []
        gathered, _ = D.compressed_all_gather(mine, codec=codec)
        res[kind, "gather_none"] = ([[_words(t) for t in per_rank] for per_rank in gathered], list(logged.log))
    dist.barrier()
    q.put((rank, res))
    dist.destroy_process_group()


def _first(log, name):
    return next(i for i, e in enumerate(log) if e[0] == name)


def test_clip_norm_and_gather_scale_world2():
    import cast_ref as R
    import scaled_ref as S

    world = 2
    inputs = [_tensor_of(r, world) for r in range(world)]
    total = (inputs[0].to(torch.float32).numpy() + inputs[1].to(torch.float32).numpy()).astype(np.float32)
    unclipped = R.cast_ref(total.view(np.uint32), R.BFLOAT16)
    wide = R.widen(unclipped, R.BFLOAT16).view(np.float32).astype(np.float64)
    assert np.isfinite(wide).all()
    # the statistic as the collective forms it: per shard in float64, the shards added in rank order
    sumsq = sum(float(np.square(wide[r * WORDS:(r + 1) * WORDS]).sum()) for r in range(world))
    norm = float(np.sqrt(sumsq))
    clip_low, clip_high = 0.5 * norm, 10.0 * norm
    coef_low = np.float32(min(clip_low / (norm + 1e-6), 1.0))
    assert 0.49 < float(coef_low) < 0.51
    clipped = S.scaled_ref(unclipped, S.BFLOAT16, coef_low)
    assert not np.array_equal(clipped, unclipped)

    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, clip_low, clip_high)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    for rank in range(world):
        res = results[rank]
        for kind in ("scaling", "plain"):
            what = f"rank {rank}, {kind} codec"
            none_words, none_log, none_coef, none_sumsq, none_keys = res[kind, "none"]
            norm_words, norm_log, _, norm_sumsq, norm_keys = res[kind, "norm"]
            low_words, low_log, low_coef, low_sumsq, low_keys = res[kind, "low"]
            high_words, high_log, high_coef, high_sumsq, high_keys = res[kind, "high"]
            # without clip_norm: the tensor, and a call log in which nothing is new
            assert np.array_equal(none_words, unclipped) and np.array_equal(norm_words, unclipped), what
            assert none_coef is None and "clip_coef" not in none_keys and "clip_coef" not in norm_keys, what
            for log in (none_log, norm_log):
                assert all(e == ("decompress", 2, ()) for e in log if e[0] == "decompress"), (what, log)
            assert not any(e[0] == "all_reduce" for e in none_log), (what, none_log)
            (stat_at,) = [i for i, e in enumerate(norm_log) if e[:2] == ("all_reduce", "torch.float64")]
            assert stat_at > max(i for i, e in enumerate(norm_log) if e[0] == "decompress"), (what, norm_log)
            assert [e for e in norm_log if e[0] != "all_reduce"] == none_log, what
            # clip_norm below the norm
            assert np.array_equal(low_words, clipped), f"{what}: the clipped tensor differs from the reference"
            assert low_coef == ("torch.float32", (), float(coef_low)), (what, low_coef, float(coef_low))
            assert abs(low_sumsq - sumsq) <= 1e-12 * sumsq and low_sumsq == norm_sumsq, what
            assert {"sumsq", "nonfinite", "global_sumsq", "global_nonfinite", "clip_coef"} <= set(low_keys), what
            (stat_at,) = [i for i, e in enumerate(low_log) if e[:2] == ("all_reduce", "torch.float64")]
            assert stat_at < _first(low_log, "decompress"), f"{what}: the statistics must be all-reduced before the gather decodes: {low_log}"
            want_decode = ("decompress", 2, ("scale",)) if kind == "scaling" else ("decompress", 2, ())
            assert all(e == want_decode for e in low_log if e[0] == "decompress"), (what, low_log)
            assert [e for e in low_log if e[0] not in ("all_reduce", "decompress")] == [e for e in none_log if e[0] != "decompress"], what
            # clip_norm above the norm: a coefficient of 1.0, and the bits of the call without it
            assert high_coef == ("torch.float32", (), 1.0), (what, high_coef)
            assert np.array_equal(high_words, none_words), what
            # compressed_all_gather(scale=...)
            third = np.float32(GATHER_SCALE)
            for key in ("gather", "gather_tensor"):
                gathered, log = res[kind, key]
                assert all(e == want_decode for e in log if e[0] == "decompress") and any(e[0] == "decompress" for e in log), (what, log)
                for r in range(world):
                    for i in range(2):
                        src = _words(inputs[r][i * WORDS:(i + 1) * WORDS])
                        assert np.array_equal(gathered[r][i], S.scaled_ref(src, S.BFLOAT16, third)), f"{what}: {key}, rank {r}'s tensor {i}"
            gathered, log = res[kind, "gather_none"]
            assert all(e == ("decompress", 2, ()) for e in log if e[0] == "decompress"), (what, log)
            for r in range(world):
                for i in range(2):
                    assert np.array_equal(gathered[r][i], _words(inputs[r][i * WORDS:(i + 1) * WORDS])), what
        # bit-identical on both ranks
    for key in (("scaling", "low"), ("plain", "low"), ("scaling", "high"), ("plain", "high")):
        assert np.array_equal(results[0][key][0], results[1][key][0]), key


def test_clip_norm_must_be_positive():
    import pytest

    from dietgpu_amd import distributed as D

    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError):
            D.compressed_all_reduce(torch.zeros(16, dtype=torch.bfloat16), codec=object(), clip_norm=bad)
