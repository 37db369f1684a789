"""The vocabulary of the call-state tests (tests/test_gpu_call_state.py, tests/test_call_state_host.py): one ITEM per C-ABI
call that uses caller temp memory or the stream's zero-at-rest counters, each on one small case.  An item knows

  run(temp, stream)  the call, enqueued on `stream` with `temp` (a uint8 CUDA tensor or None) -> its outputs as tensors,
                     plus "rc" and "used" (temp bytes the call reports); nothing here synchronises but the call itself
  expected()         the host values of those outputs, from the references the per-feature tests use (oracle, cast_ref,
                     feedback_ref, rolling_ref, reduce_cases, norm_ref), computed once
  query()            the documented temp-bytes bound of the call
  check(outs, what)  the comparison: bit for bit, except out_sumsq, which keeps norm_ref.check's bound

Sizes are words (bytes for the ANS items); a block is 4096, an encoder tile of the large geometry 8 blocks.  The cases are
the smallest shapes that reach each piece of shared state:

  rect      3 x 69637: 3 tiles each, so the rectangle is kept; element 1 is random bits (the persistent encoder's spill slots)
  ragged    163841, 36865, 300, 0, 8192: 10 of 30 tiles exist, listed by policy
  classes   ragged + 1, 4096, 777 (random bits) under dgpu_debug_set_size_classes(1): a single-block class beside the others
  pairs     1, 777, 4096, 0, 33, 4095 with 777 and 4096 random bits: the pair kernels and the spill-pool flags
  small-hw  16384, 12295, 8193 (random bits) under dgpu_debug_set_encoder_dispatch(1): hardware dispatch and the pool
  deep      one element of 65 x 32768: 65 tiles, the group words of the two-level look-back
  large     one element of 9 Mi + 123: the accumulate-by-atomics histogram in the stream's counters
  staging / tails / orders67x4   tests/reduce_cases.py, for the reduce family (orders67x4: the counts in temp memory)

This module touches no GPU state when it is imported or when expected() / query() run."""
import contextlib
import ctypes
import functools
import zlib

import numpy as np
import torch

import accum_cases as C
import cast_ref
import feedback_ref
import norm_ref
import oracle as O
import reduce_cases as R
import rolling_ref

BLK = 4096
POISON = 0xA5
THIRD = 1.0 / 3.0
PROB_BITS = 10

# name -> (sizes, elements of random bits, debug hooks set around the call)
CASES = {
    "rect": ([69637] * 3, (1,), {}),
    "ragged": ([163841, 36865, 300, 0, 8192], (), {}),
    "classes": ([163841, 36865, 300, 0, 8192, 1, 4096, 777], (7,), {"dgpu_debug_set_size_classes": 1}),
    "pairs": ([1, 777, 4096, 0, 33, 4095], (1, 2), {}),
    "small-hw": ([16384, 12295, 8193], (2,), {"dgpu_debug_set_encoder_dispatch": 1}),
    "deep": ([65 * 32768], (), {}),
    "large": ([9 * 1024 * 1024 + 123], (), {}),
}


def _rng(*key):
    return np.random.default_rng([zlib.crc32(repr(key).encode())])


@functools.lru_cache(maxsize=None)
def case_bytes(case):
    """the ANS inputs: skewed bytes, uniform ones where the case says random bits"""
    sizes, noise, _ = CASES[case]
    return [_rng(case, "u8", i).integers(0, 256, n, dtype=np.uint8) if i in noise
            else np.minimum(_rng(case, "u8", i).exponential(20.0, n), 255.0).astype(np.uint8) for i, n in enumerate(sizes)]


@functools.lru_cache(maxsize=None)
def case_bits32(case):
    """float32 bits: N(0, 1), or any 32 bits (whose bfloat16 rounding has a uniform exponent byte)"""
    sizes, noise, _ = CASES[case]
    return [_rng(case, "f32", i).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) if i in noise
            else _rng(case, "f32", i).standard_normal(n).astype(np.float32).view(np.uint32) for i, n in enumerate(sizes)]


@functools.lru_cache(maxsize=None)
def case_words(case, ft):
    """words of float type `ft`: the rounding of case_bits32, any 16 bits where the case says random bits"""
    sizes, noise, _ = CASES[case]
    if ft == O.FLOAT32:
        return case_bits32(case)
    return [_rng(case, ft, i).integers(0, 1 << 16, n, dtype=np.uint16) if i in noise else cast_ref.cast_ref(b, ft)
            for i, (n, b) in enumerate(zip(sizes, case_bits32(case)))]


@contextlib.contextmanager
def hooks(settings):
    """the library's debug hooks set for one call and put back to the policy"""
    import dietgpu_amd as dg

    L = dg.lib()
    try:
        for name, value in settings.items():
            getattr(L, name)(value)
        yield
    finally:
        for name in settings:
            getattr(L, name)(-1)


def _dev():
    return torch.device("cuda", 0)


def _stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _upload(a):
    """a numpy array as a tensor of the same bytes"""
    a = np.ascontiguousarray(a)
    kind = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.dtype.itemsize]
    signed = a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(signed.copy()).to(_dev())


def _as(t, ft):
    return t.view(C.DTYPE[ft])


def _round16(n):
    return (n + 15) // 16 * 16


def same(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.size == want.size, f"{what}: {got.size} bytes against {want.size}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ, the first at {bad[:4].tolist()}"


class Item:
    """one call on one case; see the module's text"""

    failure = False   # a documented failure outcome (status / return code), not a result
    counters = True   # the call creates the stream's counters when they do not exist yet (it uses one of the three kinds)
    calls = ()        # the C-ABI functions the item goes through

    def __init__(self, name):
        self.name = name
        self._inputs = None

    def __repr__(self):
        return self.name

    # -- to be provided
    def query(self):
        raise NotImplementedError

    def _expected(self):
        raise NotImplementedError

    def _upload_inputs(self):
        raise NotImplementedError

    def _run(self, inp, temp):
        raise NotImplementedError

    # -- shared
    def expected(self):
        if not hasattr(self, "_want"):
            self._want = self._expected()
        return self._want

    def prepare(self):
        """the inputs on the GPU, uploaded once (device synchronised: any stream may read them afterwards)"""
        if self._inputs is None:
            self._inputs = self._upload_inputs()
            torch.cuda.synchronize()
        return self._inputs

    def run(self, temp, stream=None):
        inp = self.prepare()
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            return self._run(inp, temp)

    def archive_outputs(self, n, cols):
        """[n + 1, cols] archive rows and [n + 1] sizes, poisoned; the last row is a guard"""
        return (torch.full((n + 1, _round16(max(cols, 16))), POISON, dtype=torch.uint8, device=_dev()),
                torch.full((n + 1,), -7, dtype=torch.int32, device=_dev()))

    def check_archives(self, outs, want, what, limit=None):
        comp, csizes = outs["comp"].cpu().numpy(), outs["csizes"].cpu().numpy().view(np.uint32).tolist()
        n = len(want)
        assert (comp[n] == POISON).all() and csizes[n] == 0xFFFFFFF9, f"{what}: the row behind the archives was written"
        for i, a in enumerate(want):
            assert csizes[i] == a.size, f"{what}: archive {i}: size {csizes[i]}, expected {a.size}"
            k = a.size if limit is None else min(a.size, limit)
            same(comp[i, :k], a[:k], f"{what}: archive {i}")

    def check(self, outs, what):
        want = self.expected()
        assert outs["rc"] == 0, f"{what}: rc {outs['rc']}"
        if "archives" in want:
            self.check_archives(outs, want["archives"], what)
        for key, arrays in want.get("arrays", {}).items():
            for i, (g, w) in enumerate(zip(outs[key], arrays)):
                same(g.cpu().numpy(), w, f"{what}: {key}[{i}]")
        for key, value in want.get("lists", {}).items():
            assert outs[key].cpu().tolist() == value, f"{what}: {key} {outs[key].cpu().tolist()}, expected {value}"


# ----------------------------------------------------------------------------------------------------------- encode
class AnsEncode(Item):
    def __init__(self, case, form):
        super().__init__(f"ans-encode-{form}/{case}")
        self.case, self.form = case, form
        self.op = form == "pointer"
        self.counters = case != "pairs"  # (single-block elements of raw bytes: one wavefront counts an element, nothing spills)
        self.calls = ("dgpu_ans_encode_batch_" + form,)

    def query(self):
        import dietgpu_amd as dg

        sizes = CASES[self.case][0]
        return int(dg.lib().dgpu_ans_encode_temp_bytes(len(sizes), max(sizes)))

    def _expected(self):
        return {"archives": [O.ans_encode(x, PROB_BITS, use_checksum=True) for x in case_bytes(self.case)]}

    def _upload_inputs(self):
        rows = case_bytes(self.case)
        if self.form == "pointer":
            return [_upload(x) for x in rows]
        n = rows[0].size
        assert all(r.size == n for r in rows)
        flat = np.zeros((len(rows), _round16(n)), np.uint8)
        for i, r in enumerate(rows):
            flat[i, :n] = r
        return _upload(flat)

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        sizes = CASES[self.case][0]
        n = len(sizes)
        comp, csizes = self.archive_outputs(n, O.ans_max_compressed_size(max(sizes)))
        with hooks(CASES[self.case][2]):
            if self.form == "pointer":
                _, _, used = dg.compress_data(False, inp, True, temp, comp, csizes, prob_bits=PROB_BITS)
                return {"rc": 0, "used": used, "comp": comp, "csizes": csizes}
            used = ctypes.c_size_t(0)
            rc = dg.lib().dgpu_ans_encode_batch_stride(
                _ptr(temp) if temp is not None else None, temp.numel() if temp is not None else 0, ctypes.byref(used), PROB_BITS, 1, n,
                _ptr(inp), sizes[0], _round16(sizes[0]), None, _ptr(comp), comp.size(1), _ptr(csizes), _stream_ptr())
        return {"rc": rc, "used": int(used.value), "comp": comp, "csizes": csizes}


class FloatCompress(Item):
    """dgpu_float_compress; form "capped": dgpu_float_compress_stride_capped with room for everything"""

    def __init__(self, case, ft, checksum=False, form="pointer"):
        super().__init__(f"float-compress{'-capped' if form == 'capped' else ''}-{C.DTYPE[ft]}{'-checksum' if checksum else ''}/{case}".replace("torch.", ""))
        self.case, self.ft, self.checksum, self.form = case, ft, checksum, form
        self.op = form == "pointer"
        self.calls = ("dgpu_float_compress" if form == "pointer" else "dgpu_float_compress_stride_capped",)

    def query(self):
        import dietgpu_amd as dg

        sizes = CASES[self.case][0]
        return int(dg.lib().dgpu_float_compress_temp_bytes(self.ft, len(sizes), max(sizes)))

    def _expected(self):
        return {"archives": [O.float_compress(self.ft, w, PROB_BITS, use_checksum=self.checksum) for w in case_words(self.case, self.ft)]}

    def _upload_inputs(self):
        rows = case_words(self.case, self.ft)
        if self.form == "pointer":
            return [_as(_upload(w), self.ft) for w in rows]
        assert all(r.size == rows[0].size for r in rows)
        return _upload(np.stack(rows))

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        sizes = CASES[self.case][0]
        n = len(sizes)
        comp, csizes = self.archive_outputs(n, O.float_max_compressed_size(self.ft, max(sizes)))
        with hooks(CASES[self.case][2]):
            if self.form == "pointer":
                _, _, used = dg.compress_data(True, inp, self.checksum, temp, comp, csizes, prob_bits=PROB_BITS)
                return {"rc": 0, "used": used, "comp": comp, "csizes": csizes}
            used = ctypes.c_size_t(0)
            rc = dg.lib().dgpu_float_compress_stride_capped(
                _ptr(temp) if temp is not None else None, temp.numel() if temp is not None else 0, ctypes.byref(used), self.ft, PROB_BITS,
                int(self.checksum), n, _ptr(inp), sizes[0], sizes[0] * inp.element_size(), _ptr(comp), comp.size(1), comp.size(1), _ptr(csizes),
                _stream_ptr())
        return {"rc": rc, "used": int(used.value), "comp": comp, "csizes": csizes}


class CastCompress(Item):
    calls = ("dgpu_float_cast_compress",)
    op = True

    def __init__(self, case, ft):
        super().__init__(f"cast-compress-{C.DTYPE[ft]}/{case}".replace("torch.", ""))
        self.case, self.ft = case, ft

    def query(self):
        import dietgpu_amd as dg

        sizes = CASES[self.case][0]
        return int(dg.lib().dgpu_float_compress_temp_bytes(self.ft, len(sizes), max(sizes)))

    def _expected(self):
        return {"archives": [O.float_compress(self.ft, cast_ref.cast_ref(b, self.ft), PROB_BITS) for b in case_bits32(self.case)]}

    def _upload_inputs(self):
        return [_upload(b).view(torch.float32) for b in case_bits32(self.case)]

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        sizes = CASES[self.case][0]
        comp, csizes = self.archive_outputs(len(sizes), O.float_max_compressed_size(self.ft, max(sizes)))
        with hooks(CASES[self.case][2]):
            _, _, used = dg.compress_data_cast(inp, C.DTYPE[self.ft], temp, comp, csizes, prob_bits=PROB_BITS)
        return {"rc": 0, "used": used, "comp": comp, "csizes": csizes}


class FeedbackCompress(Item):
    """fresh: no residual yet, the buffers are only written; otherwise in place on a residual of about a rounding error"""

    calls = ("dgpu_float_feedback_compress",)
    op = True

    def __init__(self, case, ft, fresh):
        super().__init__(f"feedback-compress-{'fresh' if fresh else 'in-place'}-{C.DTYPE[ft]}/{case}".replace("torch.", ""))
        self.case, self.ft, self.fresh = case, ft, fresh

    def query(self):
        import dietgpu_amd as dg

        sizes = CASES[self.case][0]
        return int(dg.lib().dgpu_float_compress_temp_bytes(self.ft, len(sizes), max(sizes)))

    @functools.cached_property
    def residual_in(self):
        out = []
        for i, x in enumerate(case_bits32(self.case)):
            e = (_rng(self.case, "residual", i).standard_normal(x.size) * 2.0 ** -9).astype(np.float32).view(np.uint32)
            out.append(feedback_ref.unambiguous(x, e))
        return out

    def _expected(self):
        arch, res = [], []
        for i, x in enumerate(case_bits32(self.case)):
            q, e, _ = feedback_ref.feedback_ref(x, None if self.fresh else self.residual_in[i], self.ft)
            arch.append(O.float_compress(self.ft, q, PROB_BITS))
            res.append(e)
        return {"archives": arch, "arrays": {"residual": res}}

    def _upload_inputs(self):
        return ([_upload(b).view(torch.float32) for b in case_bits32(self.case)],
                None if self.fresh else [_upload(e).view(torch.float32) for e in self.residual_in])

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        xs, start = inp
        sizes = CASES[self.case][0]
        comp, csizes = self.archive_outputs(len(sizes), O.float_max_compressed_size(self.ft, max(sizes)))
        if self.fresh:
            residual = [torch.full((max(n, 4),), float("nan"), dtype=torch.float32, device=_dev())[:n] for n in sizes]
        else:
            residual = [torch.cat([e, e.new_zeros(4)])[: e.numel()] for e in start]  # (a copy; never an empty allocation)
        with hooks(CASES[self.case][2]):
            _, _, used = dg.compress_data_feedback(xs, residual, C.DTYPE[self.ft], self.fresh, temp, comp, csizes, prob_bits=PROB_BITS)
        return {"rc": 0, "used": used, "comp": comp, "csizes": csizes, "residual": residual}


class RollingCompress(Item):
    """mode "out": this call's counts only; "in": coded with the counts of OTHER data; "both": one aliased buffer"""

    calls = ("dgpu_float_rolling_compress",)
    op = True

    def __init__(self, case, ft, mode):
        super().__init__(f"rolling-compress-counts-{mode}-{C.DTYPE[ft]}/{case}".replace("torch.", ""))
        self.case, self.ft, self.mode = case, ft, mode
        # (with last call's counts no histogram kernel runs; the pair encoder's spill pool has flags among the counters)
        self.counters = mode == "out" or case == "pairs"

    def query(self):
        import dietgpu_amd as dg

        sizes = CASES[self.case][0]
        return int(dg.lib().dgpu_float_compress_temp_bytes(self.ft, len(sizes), max(sizes)))

    @functools.cached_property
    def counts_in(self):
        """the exponent counts of 3 N(0, 1) data of each element's size: last step's tensor, whose distribution drifted"""
        out = []
        for i, n in enumerate(CASES[self.case][0]):
            stale = (_rng(self.case, "stale", i).standard_normal(n) * 3.0).astype(np.float32).view(np.uint32)
            out.append(rolling_ref.exponent_hist(self.ft, cast_ref.cast_ref(stale, self.ft)))
        return np.stack(out).astype(np.uint32)

    def _expected(self):
        words = case_words(self.case, self.ft)
        if self.mode == "out":
            arch = [O.float_compress(self.ft, w, PROB_BITS) for w in words]
        else:
            arch = [rolling_ref.expected_archive(self.ft, w, PROB_BITS, rolling_ref.smooth(c, w.size)) if w.size
                    else O.float_compress(self.ft, w, PROB_BITS) for w, c in zip(words, self.counts_in)]
        want = {"archives": arch}
        if self.mode != "in":
            want["arrays"] = {"counts": [np.stack([rolling_ref.exponent_hist(self.ft, w) for w in words])]}
        return want

    def _upload_inputs(self):
        return [_as(_upload(w), self.ft) for w in case_words(self.case, self.ft)], _upload(self.counts_in)

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        ts, stale = inp
        sizes = CASES[self.case][0]
        n = len(sizes)
        comp, csizes = self.archive_outputs(n, O.float_max_compressed_size(self.ft, max(sizes)))
        cin = stale.clone() if self.mode != "out" else None
        cout = cin if self.mode == "both" else (torch.full((n, 256), -0x5A5A5A5B, dtype=torch.int32, device=_dev()) if self.mode == "out" else None)
        with hooks(CASES[self.case][2]):
            _, _, used = dg.compress_data_rolling(ts, cin, cout, None, temp, comp, csizes, prob_bits=PROB_BITS)
        outs = {"rc": 0, "used": used, "comp": comp, "csizes": csizes}
        if cout is not None:
            outs["counts"] = [cout]
        return outs


# ------------------------------------------------------------------------------------------------------- reduce family
@functools.lru_cache(maxsize=None)
def reduce_sources(tag, ft):
    """-> (tests/reduce_cases.py sources, how many of them a call takes)"""
    if tag == "staging":
        return R.staging(ft), 3
    if tag == "tails":
        return R.Sources(C.tails(ft, 3), 3), 3
    if tag == "orders67x4":
        return R.orders(ft, 67, 4), 2
    raise ValueError(tag)


def _scaled(words, scale):
    with np.errstate(over="ignore", under="ignore"):
        return (np.ascontiguousarray(words, dtype=np.float32) * np.float32(scale)).astype(np.float32)


class Reduce(Item):
    """the reduce family, accumulating onto the case's starting accumulators.  compress: reduce-compress, else
    decode-reduce; variant plain / mixed (source 1 a raw row) / scaled (by a third) / norm (scaled, with both norm outputs)"""

    op = True

    def __init__(self, tag, variant, compress=True, ft=O.BFLOAT16):
        super().__init__(f"{'reduce-compress' if compress else 'decode-reduce'}-{variant}/{tag}")
        self.tag, self.variant, self.compress, self.ft = tag, variant, compress, ft
        self.counters = compress and tag != "orders67x4"  # (the counts of more than 64 members live in temp memory)
        entry = {"plain": "", "mixed": "_mixed", "scaled": "_scaled", "norm": "_norm"}[variant]
        self.calls = (("dgpu_float_reduce_compress" if compress else "dgpu_float_decode_reduce") + entry,)
        self.scale = None if variant in ("plain", "mixed") else THIRD

    def query(self):
        import dietgpu_amd as dg

        src, _ = reduce_sources(self.tag, self.ft)
        if self.variant == "norm":
            return int(dg.lib().dgpu_float_reduce_norm_temp_bytes(self.ft, len(src.sizes), max(src.sizes), int(self.compress)))
        return int(dg.lib().dgpu_float_reduce_compress_temp_bytes(self.ft, len(src.sizes), max(src.sizes)))

    def _expected(self):
        src, S = reduce_sources(self.tag, self.ft)
        sums = src.expected(S, True)
        if self.scale is not None:
            sums = [_scaled(w, self.scale) for w in sums]
        want = {"arrays": {"accs": [C.bits(w) for w in sums]}, "lists": {"status": [1] * len(src.sizes), "sizes": list(src.sizes)}}
        if self.compress:
            want["archives"] = [O.float_compress(self.ft, cast_ref.cast_ref(C.bits(w), self.ft), PROB_BITS) for w in sums]
        if self.variant == "norm":
            # reduce-compress measures the words of the ARCHIVE, decode-reduce those it leaves in the accumulator
            measured = [norm_ref.rounded(w, C.DTYPE[self.ft]) if self.compress else w for w in sums]
            want["norm"] = [norm_ref.stats(w) for w in measured]  # (exact sum of squares, non-finite count, words): once
        return want

    def _upload_inputs(self):
        src, S = reduce_sources(self.tag, self.ft)
        archives = src.archives(PROB_BITS)
        ins = [[_upload(archives[s][i]) for s in range(S)] for i in range(len(src.sizes))]
        if self.variant == "mixed":
            for i in range(len(src.sizes)):
                ins[i][1] = _as(_upload(src.words[1][i]), self.ft)
        return ins, [_upload(C.bits(w)).view(torch.float32) for w in src.start]

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        ins, start = inp
        src, _ = reduce_sources(self.tag, self.ft)
        n = len(src.sizes)
        accs = [torch.cat([a, a.new_zeros(4)])[: a.numel()] for a in start]
        status = torch.full((n,), 7, dtype=torch.uint8, device=_dev())
        sizes = torch.full((n,), -7, dtype=torch.int32, device=_dev())
        outs = {"rc": 0, "accs": accs, "status": status, "sizes": sizes}
        kw = {"prob_bits": PROB_BITS, "dtype": C.DTYPE[self.ft], "scale": self.scale}
        if self.variant == "norm":
            outs["sumsq"] = torch.full((n,), float("nan"), dtype=torch.float64, device=_dev())
            outs["nonfinite"] = torch.full((n,), -7, dtype=torch.int32, device=_dev())
            kw.update(out_sumsq=outs["sumsq"], out_nonfinite=outs["nonfinite"])
        mixed = self.variant == "mixed"
        if self.compress:
            comp, csizes = self.archive_outputs(n, O.float_max_compressed_size(self.ft, max(src.sizes)))
            f = dg.decompress_data_reduce_compress_mixed if mixed else dg.decompress_data_reduce_compress
            _, _, used = f(ins, accs, True, temp, status, sizes, comp, csizes, **kw)
            outs.update(comp=comp, csizes=csizes)
        else:
            f = dg.decompress_data_reduce_mixed if mixed else dg.decompress_data_reduce
            used = f(ins, accs, True, temp, status, sizes, **kw)
        outs["used"] = used
        return outs

    def check(self, outs, what):
        super().check(outs, what)
        if self.variant == "norm":
            # norm_ref.check's assertions -- the exact count, the sum within n * 2**-52 -- against its figures computed once
            sumsq, nonfinite = outs["sumsq"].cpu().tolist(), outs["nonfinite"].cpu().tolist()
            for i, (want, bad, n) in enumerate(self.expected()["norm"]):
                assert nonfinite[i] == bad, f"{what}: member {i}: nonfinite {nonfinite[i]}, expected {bad}"
                assert norm_ref.within(sumsq[i], want, n), f"{what}: member {i}: sumsq {sumsq[i]!r}, expected {want!r} within {n} * 2**-52"

    def repeatable(self, outs):
        """what repeats of the item must agree on bit for bit beyond the exact outputs: the 64 bits of every out_sumsq"""
        return outs["sumsq"].cpu().numpy().view(np.uint64).tolist() if self.variant == "norm" else None


# --------------------------------------------------------------------------------------------- decode with a checksum
class DecodeChecksum(Item):
    """the bounded decode with checksum=True: the only whole decode that uses temp memory (the verification scratch)"""

    counters = False
    op = True

    def __init__(self, as_float, case):
        super().__init__(f"{'float' if as_float else 'ans'}-decode-checksum/{case}")
        self.as_float, self.case, self.ft = as_float, case, O.BFLOAT16
        self.calls = ("dgpu_float_decompress_bounded",) if as_float else ("dgpu_ans_decode_batch_pointer_bounded",)

    def data(self):
        return case_words(self.case, self.ft) if self.as_float else case_bytes(self.case)

    def query(self):
        import dietgpu_amd as dg

        sizes = CASES[self.case][0]
        if self.as_float:
            return int(dg.lib().dgpu_float_decompress_temp_bytes(self.ft, len(sizes), max(sizes), PROB_BITS))
        return int(dg.lib().dgpu_ans_decode_temp_bytes(len(sizes), max(sizes), PROB_BITS))

    def archives(self):
        if self.as_float:
            return [O.float_compress(self.ft, w, PROB_BITS, use_checksum=True) for w in self.data()]
        return [O.ans_encode(x, PROB_BITS, use_checksum=True) for x in self.data()]

    def _expected(self):
        sizes = CASES[self.case][0]
        return {"arrays": {"decoded": self.data()}, "lists": {"status": [1] * len(sizes), "sizes": list(sizes)}}

    def _upload_inputs(self):
        return [_upload(a) for a in self.archives()]

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        sizes = CASES[self.case][0]
        n = len(sizes)
        word = torch.int16 if self.as_float else torch.uint8
        decoded = [torch.full((max(k, 8),), 0x5A, dtype=word, device=_dev())[:k] for k in sizes]
        status = torch.full((n,), 7, dtype=torch.uint8, device=_dev())
        osz = torch.full((n,), -7, dtype=torch.int32, device=_dev())
        outs = {"rc": 0, "decoded": decoded, "status": status, "sizes": osz, "used": 0}
        try:
            outs["used"] = dg.decompress_data(self.as_float, inp, [_as(t, self.ft) for t in decoded] if self.as_float else decoded, True, temp,
                                              status, osz, prob_bits=PROB_BITS)
        except RuntimeError as e:
            if "checksum mismatch" not in str(e):
                raise
            outs["rc"] = 3  # DGPU_ERR_CHECKSUM_MISMATCH
        return outs


# ----------------------------------------------------------------------------------------------------- failure items
class ReduceMalformed(Reduce):
    """reduce-compress of three members whose middle one has a malformed source (tests/reduce_cases.py `malformed`):
    status [1, 0, 1], the middle accumulator keeps its bits and gets a decodable archive of their rounding, the
    neighbours are summed and compressed as if it were not there"""

    failure = True
    NAME = "two 4-block tiles"

    def __init__(self):
        Item.__init__(self, "FAIL reduce-compress with a malformed source")
        self.tag, self.variant, self.compress, self.ft, self.scale = "malformed", "plain", True, O.BFLOAT16, None
        self.calls = ("dgpu_float_reduce_compress",)

    def _src(self):
        return R.malformed(self.ft, self.NAME)

    def query(self):
        import dietgpu_amd as dg

        src = self._src()
        return int(dg.lib().dgpu_float_reduce_compress_temp_bytes(self.ft, len(src.sizes), max(src.sizes)))

    def _expected(self):
        src = self._src()
        sums = src.expected(3, True)
        keep = C.bits(src.start[1])
        return {"lists": {"status": [1, 0, 1], "sizes": list(src.sizes)},
                "arrays": {"accs": [C.bits(sums[0]), keep, C.bits(sums[2])]},
                "neighbours": {k: O.float_compress(self.ft, cast_ref.cast_ref(C.bits(sums[k]), self.ft), PROB_BITS) for k in (0, 2)},
                "middle": cast_ref.cast_ref(keep, self.ft)}

    def _upload_inputs(self):
        src = self._src()
        tile_blocks, sizes, _ = C.MALFORMED_BATCHES[self.NAME]
        archives = src.archives(PROB_BITS)
        ins = [[_upload(archives[s][i]) for s in range(3)] for i in range(3)]
        what, bad = C.corruptions(self.ft, archives[1][1], sizes[1], tile_blocks)[0]
        ins[1][1] = _upload(bad)
        return ins, [_upload(C.bits(w)).view(torch.float32) for w in src.start]

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        ins, start = inp
        src = self._src()
        accs = [a.clone() for a in start]
        status = torch.full((3,), 7, dtype=torch.uint8, device=_dev())
        sizes = torch.full((3,), -7, dtype=torch.int32, device=_dev())
        comp, csizes = self.archive_outputs(3, O.float_max_compressed_size(self.ft, max(src.sizes)))
        _, _, used = dg.decompress_data_reduce_compress(ins, accs, True, temp, status, sizes, comp, csizes, prob_bits=PROB_BITS, dtype=C.DTYPE[self.ft])
        return {"rc": 0, "used": used, "accs": accs, "status": status, "sizes": sizes, "comp": comp, "csizes": csizes}

    def check(self, outs, what):
        want = self.expected()
        Item.check(self, outs, what)
        src = self._src()
        comp, csizes = outs["comp"].cpu().numpy(), outs["csizes"].cpu().numpy().view(np.uint32).tolist()
        assert (comp[3] == POISON).all(), f"{what}: the row behind the archives was written"
        for k, a in want["neighbours"].items():
            assert csizes[k] == a.size, f"{what}: archive {k}"
            same(comp[k, : a.size], a, f"{what}: archive of neighbour {k}")
        assert 0 < csizes[1] <= O.float_max_compressed_size(self.ft, src.sizes[1]), f"{what}: the failing member's archive size {csizes[1]}"
        rc, dec = O.float_decompress(self.ft, comp[1, : csizes[1]].copy(), PROB_BITS)[:2]
        assert rc == 0, f"{what}: the failing member's archive does not decode"
        same(np.asarray(dec).view(np.uint16)[: src.sizes[1]], want["middle"], f"{what}: the failing member's archive, decoded")


class RollingClipped(Item):
    """rolling compress with counts that cover nothing, at probBits 11 on just enough random words: the archive exceeds
    dgpu_float_max_compressed_size, the FULL size is reported and nothing is stored beyond the maximum"""

    failure = True
    calls = ("dgpu_float_rolling_compress",)
    op = True
    ft, P = O.BFLOAT16, 11

    def __init__(self):
        super().__init__("FAIL rolling compress clipped at the maximum")

    @functools.cached_property
    def chosen(self):
        """(words, counts): the reference alone decides which size crosses the maximum by a little"""
        hostile = rolling_ref.exponent_hist(self.ft, np.zeros(8, np.uint16)) * 1000000
        full = np.random.default_rng(7).integers(0, 1 << 16, 905 * BLK, dtype=np.uint16)
        for blocks in range(890, 906):
            n = blocks * BLK - 5
            over = rolling_ref.sizes_blockwise(self.ft, full[:n], self.P, rolling_ref.smooth(hostile, n)) - O.float_max_compressed_size(self.ft, n)
            if 16 <= over <= 4096:
                return full[:n], hostile
        raise AssertionError("no size crosses the maximum by a little")

    def query(self):
        import dietgpu_amd as dg

        return int(dg.lib().dgpu_float_compress_temp_bytes(self.ft, 1, self.chosen[0].size))

    def _expected(self):
        w, hostile = self.chosen
        full = rolling_ref.expected_archive(self.ft, w, self.P, rolling_ref.smooth(hostile, w.size))
        cap = O.float_max_compressed_size(self.ft, w.size)
        assert full.size > cap
        return {"archives": [full], "cap": cap}

    def _upload_inputs(self):
        w, hostile = self.chosen
        return [_as(_upload(w), self.ft)], _upload(hostile.astype(np.uint32).reshape(1, 256))

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        ts, cin = inp
        comp, csizes = self.archive_outputs(1, O.float_max_compressed_size(self.ft, ts[0].numel()))  # (the guard row lies right behind the maximum)
        _, _, used = dg.compress_data_rolling(ts, cin, None, None, temp, comp, csizes, prob_bits=self.P)
        return {"rc": 0, "used": used, "comp": comp, "csizes": csizes}

    def check(self, outs, what):
        want = self.expected()
        assert outs["comp"].size(1) == want["cap"]
        self.check_archives(outs, want["archives"], what, limit=want["cap"])


class CappedTooSmall(Item):
    """dgpu_float_compress_stride_capped at a width that holds the compressible rows and not the two of noise: the full
    sizes are reported, every byte below the capacity is the oracle's, nothing at or beyond it is written"""

    failure = True
    calls = ("dgpu_float_compress_stride_capped",)
    op = False
    ft, n, B, noise = O.BFLOAT16, 9 * BLK + 40, 6, (2, 5)

    def __init__(self):
        super().__init__("FAIL capped compress with too little capacity")

    @functools.cached_property
    def rows(self):
        return [_rng("capped", i).integers(0, 1 << 16, self.n, dtype=np.uint16) if i in self.noise
                else cast_ref.cast_ref(_rng("capped", i).standard_normal(self.n).astype(np.float32).view(np.uint32), self.ft) for i in range(self.B)]

    def query(self):
        import dietgpu_amd as dg

        return int(dg.lib().dgpu_float_compress_temp_bytes(self.ft, self.B, self.n))

    def _expected(self):
        arch = [O.float_compress(self.ft, r, PROB_BITS) for r in self.rows]
        width = _round16(max(a.size for i, a in enumerate(arch) if i not in self.noise) + 64)
        assert all(arch[i].size > width for i in self.noise)
        return {"archives": arch, "width": width}

    def _upload_inputs(self):
        return _upload(np.stack(self.rows))

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        width = self.expected()["width"]
        comp, csizes = self.archive_outputs(self.B, width)
        used = ctypes.c_size_t(0)
        rc = dg.lib().dgpu_float_compress_stride_capped(
            _ptr(temp) if temp is not None else None, temp.numel() if temp is not None else 0, ctypes.byref(used), self.ft, PROB_BITS, 0, self.B,
            _ptr(inp), self.n, self.n * 2, _ptr(comp), width, width, _ptr(csizes), _stream_ptr())
        return {"rc": rc, "used": int(used.value), "comp": comp, "csizes": csizes}

    def check(self, outs, what):
        want = self.expected()
        assert outs["rc"] == 0 and outs["comp"].size(1) == want["width"]
        self.check_archives(outs, want["archives"], what, limit=want["width"])  # (a row's first byte beyond the capacity is the next row's)
        comp = outs["comp"].cpu().numpy()
        for i, a in enumerate(want["archives"]):
            assert (comp[i, min(_round16(a.size), want["width"]):] == POISON).all(), f"{what}: row {i} was written behind its archive"


class HistogramTooNarrow(Item):
    """dgpu_ans_encode_batch_pointer with a caller's histogram that does not cover the middle element: that element is
    reported as failed (size 0), its neighbours are the oracle's archives under their histograms"""

    failure = True
    counters = False
    calls = ("dgpu_ans_encode_batch_pointer",)
    op = False
    n = BLK * 20 + 7

    def __init__(self):
        super().__init__("FAIL caller histogram that does not cover the data")

    @functools.cached_property
    def rows(self):
        good = np.minimum(_rng("hist", 0).exponential(50.0, self.n), 255.0).astype(np.uint8)
        return [good, _rng("hist", 1).integers(0, 256, self.n, dtype=np.uint8), good[::-1].copy()]

    @functools.cached_property
    def hist(self):
        counts = np.stack([np.bincount(r, minlength=256) for r in self.rows]).astype(np.uint32)
        counts[1] = 0
        counts[1][0] = self.n  # "all zeros": 255 of the 256 symbols of the middle row are not covered
        return counts

    def query(self):
        import dietgpu_amd as dg

        return int(dg.lib().dgpu_ans_encode_temp_bytes(3, self.n))

    def _expected(self):
        return {"neighbours": {i: O.ans_encode(self.rows[i], PROB_BITS, counts=self.hist[i]) for i in (0, 2)}}

    def _upload_inputs(self):
        return [_upload(r) for r in self.rows], _upload(self.hist)

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        rows, hist = inp
        comp, csizes = self.archive_outputs(3, O.ans_max_compressed_size(self.n))
        used = ctypes.c_size_t(0)
        rc = dg.lib().dgpu_ans_encode_batch_pointer(
            _ptr(temp) if temp is not None else None, temp.numel() if temp is not None else 0, ctypes.byref(used), PROB_BITS, 0, 3,
            (ctypes.c_void_p * 3)(*[t.data_ptr() for t in rows]), (ctypes.c_uint32 * 3)(*[self.n] * 3), _ptr(hist),
            (ctypes.c_void_p * 3)(*[comp[i].data_ptr() for i in range(3)]), _ptr(csizes), _stream_ptr())
        return {"rc": rc, "used": int(used.value), "comp": comp, "csizes": csizes}

    def check(self, outs, what):
        assert outs["rc"] == 0, what
        comp, csizes = outs["comp"].cpu().numpy(), outs["csizes"].cpu().numpy().view(np.uint32).tolist()
        assert (comp[3] == POISON).all(), f"{what}: the row behind the archives was written"
        assert csizes[1] == 0, f"{what}: the element the histogram does not cover reports size {csizes[1]}"
        for i, a in self.expected()["neighbours"].items():
            assert csizes[i] == a.size, f"{what}: archive {i}"
            same(comp[i, : a.size], a, f"{what}: archive of neighbour {i}")


class ChecksumFlipped(DecodeChecksum):
    """the ANS decode of `rect` with the stored checksum of member 1 flipped: DGPU_ERR_CHECKSUM_MISMATCH (the tensor
    surface raises), the data decoded all the same"""

    failure = True

    def __init__(self):
        super().__init__(False, "rect")
        self.name = "FAIL decode with a flipped stored checksum"

    def archives(self):
        out = [a.copy() for a in super().archives()]
        out[1][20] ^= 0x5A  # ANSCoalescedHeader::checksum
        return out

    def check(self, outs, what):
        assert outs["rc"] == 3, f"{what}: rc {outs['rc']}, expected DGPU_ERR_CHECKSUM_MISMATCH"
        outs = dict(outs, rc=0)
        super().check(outs, what)


class ProbBitsRejected(Item):
    """probBits = 12: DGPU_ERR_INVALID_ARGUMENT before anything is enqueued -- no output byte is touched"""

    failure = True
    counters = False
    calls = ("dgpu_float_compress",)
    op = False

    def __init__(self):
        super().__init__("FAIL probBits 12 rejected")

    def query(self):
        import dietgpu_amd as dg

        sizes = CASES["rect"][0]
        return int(dg.lib().dgpu_float_compress_temp_bytes(O.BFLOAT16, len(sizes), max(sizes)))

    def _expected(self):
        return {"rc": 1}

    def _upload_inputs(self):
        return [_as(_upload(w), O.BFLOAT16) for w in case_words("rect", O.BFLOAT16)]

    def _run(self, inp, temp):
        import dietgpu_amd as dg

        sizes = CASES["rect"][0]
        comp, csizes = self.archive_outputs(len(sizes), O.float_max_compressed_size(O.BFLOAT16, max(sizes)))
        rc = 0
        try:
            dg.compress_data(True, inp, False, temp, comp, csizes, prob_bits=12)
        except dg.DietGpuError as e:
            rc = int(str(e).split("error ")[1].split(":")[0])
        return {"rc": rc, "used": 0, "comp": comp, "csizes": csizes}

    def check(self, outs, what):
        assert outs["rc"] == 1, f"{what}: rc {outs['rc']}, expected DGPU_ERR_INVALID_ARGUMENT"
        assert bool((outs["comp"] == POISON).all()) and bool((outs["csizes"] == -7).all()), f"{what}: an output was written"


# ----------------------------------------------------------------------------------------------------- the vocabulary
def _items():
    bf, h, f32 = O.BFLOAT16, O.FLOAT16, O.FLOAT32
    out = [AnsEncode(case, "pointer") for case in ("rect", "ragged", "classes", "pairs", "small-hw")]
    out += [AnsEncode("rect", "stride")]
    out += [FloatCompress(case, bf) for case in ("rect", "ragged", "classes", "pairs", "small-hw", "deep", "large")]
    out += [FloatCompress("rect", bf, checksum=True), FloatCompress("rect", h), FloatCompress("pairs", h), FloatCompress("rect", f32),
            FloatCompress("ragged", f32), FloatCompress("rect", bf, form="capped")]
    out += [CastCompress(case, bf) for case in ("rect", "ragged", "classes", "pairs", "small-hw", "deep", "large")]
    out += [CastCompress("rect", h)]
    # (feedback takes no null entry in its pointer arrays, and an empty tensor has no address: the cases without one)
    out += [FeedbackCompress("rect", bf, True), FeedbackCompress("small-hw", bf, True), FeedbackCompress("rect", bf, False),
            FeedbackCompress("small-hw", h, False)]
    out += [RollingCompress("rect", bf, "out"), RollingCompress("ragged", bf, "out"), RollingCompress("rect", bf, "in"),
            RollingCompress("pairs", bf, "in"), RollingCompress("rect", bf, "both"), RollingCompress("small-hw", h, "both")]
    out += [Reduce(tag, "plain") for tag in ("staging", "tails", "orders67x4")]
    out += [Reduce("staging", "mixed"), Reduce("staging", "scaled"), Reduce("orders67x4", "scaled")]
    out += [Reduce(tag, "norm") for tag in ("staging", "tails", "orders67x4")]
    out += [Reduce("staging", "norm", compress=False), Reduce("orders67x4", "norm", compress=False)]
    out += [DecodeChecksum(False, "rect"), DecodeChecksum(True, "ragged")]
    return out


ITEMS = _items()
FAILURES = [ReduceMalformed(), RollingClipped(), CappedTooSmall(), HistogramTooNarrow(), ChecksumFlipped(), ProbBitsRejected()]
BY_NAME = {i.name: i for i in ITEMS + FAILURES}
assert len(BY_NAME) == len(ITEMS) + len(FAILURES)

# Functions of include/dietgpu_amd.h with a `temp_dev` parameter that the vocabulary leaves out, and why.
ALLOWED = {
    # same implementation behind another description of the batch (capi.hip: every form resolves to encodeBatch / decodeImpl)
    "dgpu_ans_encode_batch_split_size": "encodeBatch, as the pointer and stride forms in the vocabulary",
    "dgpu_float_compress_split_size": "encodeBatch, as dgpu_float_compress",
    "dgpu_ans_decode_batch_stride": "decodeImpl, as dgpu_ans_decode_batch_pointer_bounded",
    "dgpu_ans_decode_batch_pointer": "decodeImpl, as dgpu_ans_decode_batch_pointer_bounded",
    "dgpu_ans_decode_batch_split_size": "decodeImpl, as dgpu_ans_decode_batch_pointer_bounded",
    "dgpu_ans_decode_batch_split_size_bounded": "decodeImpl, as dgpu_ans_decode_batch_pointer_bounded",
    "dgpu_float_decompress": "decodeImpl, as dgpu_float_decompress_bounded",
    "dgpu_float_decompress_split_size": "decodeImpl, as dgpu_float_decompress_bounded",
    "dgpu_float_decompress_split_size_bounded": "decodeImpl, as dgpu_float_decompress_bounded",
    "dgpu_float_decompress_stride_bounded": "decodeImpl, as dgpu_float_decompress_bounded",
    # temp_dev is accepted for symmetry and never used
    "dgpu_ans_get_compressed_info": "reads headers only: no temp memory, no counters",
    "dgpu_float_get_compressed_info": "reads headers only: no temp memory, no counters",
}
# ... and the decode forms whose documentation says "No temp memory is used": the GPU test asserts *tempUsed == 0 once
NO_TEMP = ("dgpu_ans_decode_batch_pointer_range", "dgpu_float_decompress_range", "dgpu_float_decode_accumulate",
           "dgpu_float_decode_accumulate_scaled", "dgpu_float_decode_scaled", "dgpu_float_decode_reduce",
           "dgpu_float_decode_reduce_mixed", "dgpu_float_decode_reduce_scaled")
