"""compressed_all_reduce(out=, out_scale=, out_accumulate=) on CPU: two gloo ranks, the CPU oracle as the codec, in three
shapes -- a `decompress_accumulate` with a `scale` parameter (it applies tests/accum_scaled_ref.py), one without, and a
codec without `decompress_accumulate` at all -- on a float32 tensor with wire_dtype=bfloat16, a bfloat16 tensor and a
float16 tensor.  Under test is the plumbing: the float32 result has the same bits on both ranks, with every codec, as the
numpy reference; the factor reaches the decode; and with out=None every codec call is the one it always was."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_accumulate_gloo import ROOT, WORDS, _free_port

KINDS = ("f32 on bf16", "bf16", "fp16")
CODECS = ("scaled", "plain", "decode only")
OUT_SCALE = -0.0625 * 1.1


def _input(kind, rank, world):
    g = torch.Generator().manual_seed(900 + 10 * KINDS.index(kind) + rank)
    x = torch.randn(world * WORDS, generator=g)
    return x if kind == "f32 on bf16" else x.to(torch.bfloat16 if kind == "bf16" else torch.float16)


def _wire(kind):
    return torch.float16 if kind == "fp16" else torch.bfloat16


def _ft(dtype):
    return 1 if dtype == torch.float16 else 2


def _np16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def _bits32(t):
    return t.contiguous().numpy().view(np.uint32).copy()


class _Codec:
    """the CPU oracle behind the codec interface of the collectives, for float16 and bfloat16 rows; every call is logged
    as (name, positional arguments, keyword names)"""

    def __init__(self, O, log):
        self.O, self.log, self.ft = O, log, None

    def _compress(self, tensors):
        O = self.O
        self.ft = _ft(tensors[0].dtype)
        arch = [O.float_compress(self.ft, _np16(t), 10) for t in tensors]
        cap = max(O.float_max_compressed_size(self.ft, t.numel()) for t in tensors)
        comp = torch.zeros((len(arch), cap), dtype=torch.uint8)
        for i, a in enumerate(arch):
            comp[i, : a.size] = torch.from_numpy(a.copy())
        return comp, torch.tensor([a.size for a in arch], dtype=torch.int32)

    def compress(self, tensors):
        self.log.append(("compress", 1, ()))
        return self._compress(tensors)

    def compress_cast(self, tensors, dtype):
        import cast_ref as R

        self.log.append(("compress_cast", 2, ()))
        assert all(t.dtype == torch.float32 for t in tensors)
        return self._compress([torch.from_numpy(R.cast_ref(_bits32(t), _ft(dtype)).view(np.int16)).view(dtype) for t in tensors])

    def _words(self, row, n):
        rc, w, _ = self.O.float_decompress(self.ft, row.numpy(), 10, n)
        assert rc == 0 and w.size == n
        return w

    def _accumulate(self, rows, accs, accumulate, factor):
        import accum_scaled_ref as A

        for r, acc in zip(rows, accs):
            w = self._words(r, acc.numel())
            if factor is None:
                got = A.widen(w, self.ft).view(np.uint32) if not accumulate else A.accum_scaled_ref(w, self.ft, 1.0, _bits32(acc))
            else:
                got = A.accum_scaled_ref(w, self.ft, np.float32(float(factor)), _bits32(acc) if accumulate else None)
            acc.copy_(torch.from_numpy(got.view(np.float32).copy()))
        return torch.ones((len(rows),), dtype=torch.uint8)

    def decompress(self, *args, **kwargs):
        self.log.append(("decompress", len(args), tuple(sorted(kwargs))))
        rows, outs = args
        assert not kwargs
        for r, out in zip(rows, outs):
            out.view(torch.int16).copy_(torch.from_numpy(self._words(r, out.numel()).view(np.int16).copy()))
        return torch.ones((len(rows),), dtype=torch.uint8)


class _ScaledCodec(_Codec):
    def decompress_accumulate(self, rows, accs, accumulate, scale=None):
        self.log.append(("decompress_accumulate", 3, () if scale is None else ("scale",)))
        if scale is not None:
            assert isinstance(scale, torch.Tensor) and scale.dtype == torch.float32 and scale.dim() == 0
        return self._accumulate(rows, accs, accumulate, scale)


class _PlainCodec(_Codec):
    def decompress_accumulate(self, *args, **kwargs):
        self.log.append(("decompress_accumulate", len(args), tuple(sorted(kwargs))))
        assert not kwargs
        rows, accs, accumulate = args
        return self._accumulate(rows, accs, accumulate, None)


class _DecodeOnlyCodec(_Codec):
    """no decompress_accumulate: the reduce-scatter sums through decompress_reduce"""

    def decompress_reduce(self, rows_per_acc, accs, accumulate):
        self.log.append(("decompress_reduce", 3, ()))
        for rows, acc in zip(rows_per_acc, accs):
            for k, r in enumerate(rows):
                self._accumulate([r], [acc], accumulate or k > 0, None)
        return torch.ones((len(accs),), dtype=torch.uint8)


_CODEC = {"scaled": _ScaledCodec, "plain": _PlainCodec, "decode only": _DecodeOnlyCodec}


def _prefill(world):
    g = torch.Generator().manual_seed(77)
    return torch.randn(world * WORDS, generator=g) * 3.0


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
        base = {} if x.dtype != torch.float32 else {"wire_dtype": _wire(kind)}
        clip = clips[kind]
        for name in CODECS:
            log = []
            codec = _CODEC[name](O, log)

            def run(**kwargs):
                del log[:]
                t = kwargs.pop("tensor", None)
                out, stats = D.compressed_all_reduce(x.clone() if t is None else t, codec=codec, **base, **kwargs)
                coef = stats.get("clip_coef")
                return out, list(log), None if coef is None else float(coef), sorted(stats)

            r = {}
            out, r["today log"], _, _ = run()
            r["today"] = _np16(out)
            out, r["today clip log"], r["coef"], _ = run(clip_norm=clip)
            r["today clip"] = _np16(out)
            empty = lambda: torch.full((world * WORDS,), float("nan"))
            for case, kwargs in (
                ("i", {}),
                ("ii", {"clip_norm": clip}),
                ("iii number", {"out_scale": OUT_SCALE}),
                ("iii tensor", {"out_scale": torch.tensor([OUT_SCALE], dtype=torch.float32)}),
                ("iii number clip", {"out_scale": OUT_SCALE, "clip_norm": clip}),
                ("iii tensor clip", {"out_scale": torch.tensor(OUT_SCALE, dtype=torch.float32), "clip_norm": clip}),
                ("iv", {"out_scale": OUT_SCALE, "clip_norm": clip, "out_accumulate": True}),
                ("iv plain", {"out_accumulate": True}),
            ):
                buf = _prefill(world) if kwargs.get("out_accumulate") else empty()
                out, lg, coef, keys = run(out=buf, **kwargs)
                assert out is buf
                r[case] = (_bits32(buf), lg, coef, keys)
            if x.dtype == torch.float32:
                t = x.clone()
                out, lg, coef, keys = run(tensor=t, out=t, out_scale=OUT_SCALE)
                assert out is t
                r["v"] = (_bits32(t), lg, coef, keys)
            res[kind, name] = r
    dist.barrier()
    q.put((rank, res))
    dist.destroy_process_group()


def _archive_words(kind, world):
    """the 16-bit words of the all-reduce's archives: the float32 sum in rank order of the exactly widened (wire-rounded)
    inputs, rounded once"""
    import accum_scaled_ref as A
    import cast_ref as R

    ft = _ft(_wire(kind))
    total = None
    for r in range(world):
        x = _input(kind, r, world)
        w16 = R.cast_ref(_bits32(x), ft) if x.dtype == torch.float32 else _np16(x)
        wide = A.widen(w16, ft)
        total = wide.copy() if total is None else (total + wide).astype(np.float32)
    return R.cast_ref(np.ascontiguousarray(total).view(np.uint32), ft), ft


def test_float32_out_world2():
    import accum_scaled_ref as A
    import cast_ref as R

    world = 2
    words, clips = {}, {}
    for kind in KINDS:
        w, ft = _archive_words(kind, world)
        wide = A.widen(w, ft).astype(np.float64)
        assert np.isfinite(wide).all()
        norm = float(np.sqrt(sum(float(np.square(wide[r * WORDS:(r + 1) * WORDS]).sum()) for r in range(world))))
        words[kind], clips[kind] = (w, ft, norm), 0.5 * norm

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

    pre = _bits32(_prefill(world))
    f32 = np.float32
    for kind in KINDS:
        w, ft, norm = words[kind]
        wire = kind == "f32 on bf16"
        coef = f32(results[0][kind, "scaled"]["coef"])
        # clip_grad_norm_'s coefficient, as the collective computes it today; the reference takes the value it reports
        assert abs(float(coef) - min(clips[kind] / (norm + 1e-6), 1.0)) <= 1e-6 and 0.49 < float(coef) < 0.51
        scale = f32(OUT_SCALE)
        both = f32(coef * scale)  # one float32 multiply
        want = {
            "i": R.widen(w, ft),
            "ii": A.accum_scaled_ref(w, ft, coef),
            "iii number": A.accum_scaled_ref(w, ft, scale),
            "iii tensor": A.accum_scaled_ref(w, ft, scale),
            "iii number clip": A.accum_scaled_ref(w, ft, both),
            "iii tensor clip": A.accum_scaled_ref(w, ft, both),
            "iv": A.accum_scaled_ref(w, ft, both, pre),
            "iv plain": A.accum_scaled_ref(w, ft, 1.0, pre),
            "v": A.accum_scaled_ref(w, ft, scale),
        }
        for rank in range(world):
            for name in CODECS:
                r = results[rank][kind, name]
                what = f"{kind}, rank {rank}, {name} codec"
                assert f32(r["coef"]) == coef, what
                # today's 16-bit results, and what the float32 results must be beside them
                assert np.array_equal(r["today"], w), what
                assert np.array_equal(r["i"][0], R.widen(r["today"], ft)), f"{what}: (i) is not today's result .float()"
                assert np.array_equal(R.cast_ref(r["ii"][0], ft), r["today clip"]), f"{what}: (ii).to(dtype) is not today's clipped result"
                for case, bits in want.items():
                    if case == "v" and not wire:
                        continue
                    got, log, got_coef, keys = r[case]
                    assert np.array_equal(got, bits), f"{what}: case {case} differs from the reference"
                    assert not A.is_nan(got).any(), what
                    assert (got_coef is not None) == ("clip" in case or case in ("ii", "iv")), (what, case)
                    if got_coef is not None:
                        assert f32(got_coef) == coef and "clip_coef" in keys and "global_sumsq" in keys, (what, case)
                    # the codec calls of the gather: the ones behind the shard's archive
                    tail = log[max(i for i, e in enumerate(log) if e[0] == "compress_cast") + 1:]
                    factor = case not in ("i", "iv plain")
                    if name == "scaled":
                        assert tail == [("decompress_accumulate", 3, ("scale",) if factor else ())] * world, (what, case, tail)
                        assert not any(e[0] == "decompress" for e in log), (what, case, log)
                    elif name == "plain":
                        assert tail == [("decompress_accumulate", 3, ())] * world, (what, case, tail)
                        assert not any(e[0] == "decompress" for e in log), (what, case, log)
                    else:
                        assert tail == [("decompress", 2, ())] * world, (what, case, tail)
                    # ... and nothing else moved
                    head = r["today log"][: len(r["today log"]) - world]
                    assert log[: len(log) - world] == head, (what, case, log)
                # out=None: every codec call is the one it always was
                first = ("compress_cast", 2, ()) if wire else ("compress", 1, ())
                reduce = [("decompress_reduce", 3, ())] if name == "decode only" else [("decompress_accumulate", 3, ())] * world
                always = [first] + reduce + [("compress_cast", 2, ())] + [("decompress", 2, ())] * world
                assert r["today log"] == always and r["today clip log"] == always, (what, r["today log"], r["today clip log"])
        for name in CODECS:
            for case in want:
                if case == "v" and not wire:
                    continue
                assert np.array_equal(results[0][kind, name][case][0], results[1][kind, name][case][0]), (kind, name, case)
                assert np.array_equal(results[0][kind, name][case][0], results[0][kind, "scaled"][case][0]), (kind, name, case)


def test_argument_errors():
    from dietgpu_amd import distributed as D

    bf = torch.zeros(16, dtype=torch.bfloat16)
    f32 = torch.zeros(16, dtype=torch.float32)
    ok = torch.zeros(16, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="need `out`"):
        D.compressed_all_reduce(bf, codec=object(), out_scale=0.5)
    with pytest.raises(RuntimeError, match="need `out`"):
        D.compressed_all_reduce(bf, codec=object(), out_accumulate=True)
    with pytest.raises(RuntimeError, match="out_accumulate"):
        D.compressed_all_reduce(f32, codec=object(), wire_dtype=torch.bfloat16, out=f32, out_accumulate=True)
    for bad in (torch.zeros(16, dtype=torch.bfloat16), torch.zeros(15), torch.zeros(4, 4), torch.zeros(32)[::2], "out"):
        with pytest.raises(RuntimeError, match="flat contiguous float32"):
            D.compressed_all_reduce(bf, codec=object(), out=bad)
    for bad in (0.0, float("inf"), float("nan"), 1e-60):
        with pytest.raises(RuntimeError, match="finite and not zero"):
            D.compressed_all_reduce(bf, codec=object(), out=ok, out_scale=bad)
    for bad in (torch.ones(2), torch.ones(1, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="0-dim or 1-element float32"):
            D.compressed_all_reduce(bf, codec=object(), out=ok, out_scale=bad)
