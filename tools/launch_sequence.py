#!/usr/bin/env python3
"""A fixed list of compress + decompress calls that reaches every branch of the kernel selection
(csrc/kernel_variants.h), and the digest of the launches a profiler saw them make.  Two builds of the library select
the same kernels when their digests agree:

    rocprofv3 --kernel-trace -d DIR -o seq -- python tools/launch_sequence.py --temp-out DIR/temp.txt   (once per build)
    python tools/launch_sequence.py --digest DIR/seq_results.db --temp DIR/temp.txt [--lines OUT.txt]

The calls: raw bytes, fp16, bf16 and fp32; probBits 9, 10 and 11; elements of one block (the pair kernels) and tiles
of 2, 4 and 8 blocks, the 8-block ones with at most 32 tiles per element (wide stage) and with more; the encoder's
dispatch left to the policy, forced persistent and forced to the hardware; ordinary histogram loads; one batch of size
classes (1 large + many small) and one ragged batch; a caller-supplied histogram; ranged decodes on 16-block and 4-block
tiles and of nothing but empty requests; decode-accumulate as a rectangle and from a list; cast-compress as a rectangle,
ragged and split into classes that hold single-block members; the reduce family (REDUCE_SHAPES, reduce_family below) on
the ctypes route and on the torch route; stochastic cast-compress on both routes, last (stochastic_compress below: the
lines of the calls before it do not move).  The digest is over the lines (kernel name with its
template arguments, grid, workgroup size, LDS bytes) in launch order and, with --temp, the temp bytes every call of the
list reported (tempUsed), in call order."""
import argparse
import ctypes as C
import hashlib
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (words per element, elements): one block; tiles of 2 / 4 blocks, more of them than fit on the chip at once; 8-block
# tiles with 4 tiles per element; with 40 tiles per element, more tiles than resident workgroups
SHAPES = [(3000, 64), (8000, 2048), (16000, 2048), (100000, 16), (40 * 32768, 64)]


# The reduce family's batches (words per member): one 4-block tile each; two 16-block tiles each; a ragged batch that
# planDecodeCall turns into a tile list ("equal_tiles_other_sizes" of tests/cpp/plan_dump.cpp); more members than
# kAccElements (64), so that reduce-compress takes its counts, and the norm its partials, from temp memory.
REDUCE_SHAPES = {
    "4block": [8000] * 3,
    "16block": [70000] * 3,
    "ragged": [40000, 60000, 50000, 65536, 33000, 300000, 120000, 70000, 131072, 66000],
    "b65": [8000] * 65,
}


def digest(db, lines_out, temp):
    con = sqlite3.connect(db)
    cols = [d[1] for d in con.execute("pragma table_info(kernels)")]
    want = [c for c in ("name", "grid_x", "grid_y", "workgroup_x", "lds_size") if c in cols]
    rows = con.execute(f"select {', '.join(want)} from kernels where name like '%dgpu::%' order by start").fetchall()
    lines = [" ".join(str(x) for x in r) for r in rows]
    launches = len(lines)
    if temp:
        lines += open(temp).read().splitlines()
    if lines_out:
        with open(lines_out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(f"{launches} launches, {len(set(lines[:launches]))} distinct, {len(lines) - launches} tempUsed lines, sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}")


def main(temp_out):
    import torch

    import dietgpu_amd as dg

    L = dg.lib()
    dg.ops.prefer_torch_ops(False)  # (prob_bits and the debug setters act on the core library: one route for all)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)

    def tensors(dtype, sizes):
        if dtype == torch.uint8:
            return [(torch.randn([n], generator=g, device=dev) * 12).to(torch.int8).view(torch.uint8) for n in sizes]
        return [torch.randn([n], generator=g, device=dev).to(dtype) for n in sizes]

    temp_lines = []

    def used(what, nbytes):
        temp_lines.append(f"tempUsed {len(temp_lines)} {what} {nbytes}")
        print(temp_lines[-1])

    def rows_of(comp, sizes):
        return [comp[i, : int(s)] for i, s in enumerate(sizes.tolist())]

    def round_trip(ts, prob_bits):
        is_float = ts[0].dtype != torch.uint8
        comp, sizes, temp = dg.compress_data(is_float, ts, False, prob_bits=prob_bits)
        used("compress", temp)
        outs = [torch.empty_like(t) for t in ts]
        used("decompress", dg.decompress_data(is_float, rows_of(comp, sizes), outs, False, prob_bits=prob_bits))
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(ts, outs)), "round trip mismatch"
        return comp, sizes

    dtypes = (torch.uint8, torch.float16, torch.bfloat16, torch.float32)
    for dtype in dtypes:
        for words, batch in SHAPES:
            ts = list(tensors(dtype, [words * batch])[0].view(batch, words).unbind(0))
            for prob_bits in (9, 10, 11):
                for dispatch in (-1, 0, 1):
                    L.dgpu_debug_set_encoder_dispatch(dispatch)
                    round_trip(ts, prob_bits)
            L.dgpu_debug_set_encoder_dispatch(-1)
            L.dgpu_set_histogram_load_policy(1)
            round_trip(ts, 10)
            L.dgpu_set_histogram_load_policy(-1)
    for dtype in (torch.uint8, torch.bfloat16):
        round_trip(tensors(dtype, [2 * 1024 * 1024] + [1000 + 37 * i for i in range(200)]), 10)  # size classes
        round_trip(tensors(dtype, [64 * 1024 + 15000 * i for i in range(64)]), 10)  # ragged

    # caller-supplied histogram (stand-alone normalisation)
    n, b = 50000, 4
    x = tensors(torch.uint8, [n * b])[0]
    hist = torch.zeros([b, 256], dtype=torch.int32, device=dev)
    stride = int(L.dgpu_ans_max_compressed_size(n))
    arch = torch.zeros([b, stride], dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.dgpu_ans_histogram_batch_stride(b, p(x), n, n, p(hist), st) == 0
    assert L.dgpu_ans_encode_batch_stride(None, 0, None, 10, 0, b, p(x), n, n, p(hist), p(arch), stride, None, st) == 0
    out = torch.empty_like(x)
    assert L.dgpu_ans_decode_batch_stride(None, 0, None, 10, 0, b, p(arch), stride, p(out), n, n, None, None, st, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, x), "round trip mismatch (caller-supplied histogram)"

    # ranged decode: ranges of up to 20 blocks (16-block tiles), of up to 8 (4-block tiles), nothing but empty requests
    ts = tensors(torch.bfloat16, [40 * 4096 - 100 * i for i in range(12)])
    comp, sizes = round_trip(ts, 10)
    for first, num in (([i % 5 for i in range(12)], [20 - i for i in range(12)]), ([i for i in range(12)], [1 + i % 8 for i in range(12)]),
                       ([0] * 12, [0] * 12)):
        outs = [torch.zeros([max(n, 1) * 4096], dtype=torch.bfloat16, device=dev) for n in num]
        used("decompress_range", dg.decompress_data_range(True, rows_of(comp, sizes), outs, first, num, prob_bits=10))
        for t, o, f, n in zip(ts, outs, first, num):
            want = t[f * 4096 : (f + n) * 4096]
            assert torch.equal(o[: want.numel()].view(torch.int16), want.view(torch.int16)), "ranged decode mismatch"

    # decode-accumulate: equal capacities (the rectangle), capacities that differ widely (the list)
    for words in ([100000] * 16, [64 * 1024 + 15000 * i for i in range(64)]):
        ts = tensors(torch.bfloat16, words)
        comp, sizes = round_trip(ts, 10)
        accs = [torch.ones([n], dtype=torch.float32, device=dev) for n in words]
        used("decompress_accumulate", dg.decompress_data_accumulate(rows_of(comp, sizes), accs, True, prob_bits=10, dtype=torch.bfloat16))
        assert all(torch.equal(a, t.float() + 1) for a, t in zip(accs, ts)), "decode-accumulate mismatch"

    # cast-compress: the rectangle, a ragged batch, size classes with single-block members (they run on 2-block tiles)
    for words in ([100000] * 16, [64 * 1024 + 15000 * i for i in range(64)], [2 * 1024 * 1024] + [1000 + 37 * i for i in range(300)]):
        ts = tensors(torch.float32, words)
        comp, sizes, temp = dg.compress_data_cast(ts, torch.bfloat16, prob_bits=10)
        used("compress_cast", temp)
        outs = [torch.empty([n], dtype=torch.bfloat16, device=dev) for n in words]
        used("decompress", dg.decompress_data(True, rows_of(comp, sizes), outs, False, prob_bits=10))
        assert all(torch.equal(o.view(torch.int16), t.to(torch.bfloat16).view(torch.int16)) for o, t in zip(outs, ts)), "cast-compress mismatch"
    reduce_family(dg, torch, tensors, rows_of, used)
    stochastic_compress(dg, torch, tensors, rows_of)
    if temp_out:
        with open(temp_out, "w") as f:
            f.write("\n".join(temp_lines) + "\n")
    print("launch sequence done")


def reduce_family(dg, torch, tensors, rows_of, used):
    """Decode-accumulate, scaled decompress and the eight reduce calls, each on both routes: S = 1 and 2; bf16 and fp16
    (fp32: decode-reduce only); every form -- plain, mixed with and without a raw row, scale 1/3 and 1.0, norm with both
    outputs (scaled), with one, and with scale 1.0; probBits 10, and 11 for one batch."""
    dev = torch.device("cuda:0")
    third = 1.0 / 3.0
    s32 = torch.tensor(third, dtype=torch.float32).item()
    # (keywords of the call beyond the sources; whether source S-1 of member 0 is passed as a raw row)
    forms = [("plain", {}, False), ("mixed_raw", {}, True), ("mixed_archives", {}, None), ("scale_third", {"scale": third}, False),
             ("scale_one", {"scale": 1.0}, False), ("norm_both", {"scale": third, "sumsq": True, "nonfinite": True}, False),
             ("norm_one", {"nonfinite": True}, False), ("norm_scale_one", {"scale": 1.0, "sumsq": True, "nonfinite": True}, False)]

    def sources(dtype, words, prob_bits):
        ts = [tensors(dtype, words) for _ in range(2)]
        rows = []
        for t in ts:
            comp, sizes, temp = dg.compress_data(True, t, False, prob_bits=prob_bits)
            used("compress", temp)
            rows.append(rows_of(comp, sizes))
        return ts, rows

    def reduce_calls(route, dtype, shape, ts, rows, prob_bits, compress):
        words, n = REDUCE_SHAPES[shape], len(ts[0])
        for S in (1, 2):
            total = ts[0] if S == 1 else [a.float() + b.float() for a, b in zip(ts[0], ts[1])]
            for name, kw, raw in forms:
                src = [[rows[s][i] for s in range(S)] for i in range(n)]
                if raw:
                    src[0][S - 1] = ts[S - 1][0]
                accs = [torch.full([w], 7.0, dtype=torch.float32, device=dev) for w in words]
                status = torch.zeros([n], dtype=torch.uint8, device=dev)
                extra = {"scale": kw["scale"]} if "scale" in kw else {}
                if kw.get("sumsq"):
                    extra["out_sumsq"] = torch.zeros([n], dtype=torch.float64, device=dev)
                if kw.get("nonfinite"):
                    extra["out_nonfinite"] = torch.ones([n], dtype=torch.int32, device=dev)
                mixed = raw is not False
                fn = getattr(dg, "decompress_data_reduce" + ("_compress" if compress else "") + ("_mixed" if mixed else ""))
                out = fn(src, accs, False, None, status, None, prob_bits=prob_bits, dtype=dtype, **extra)
                used(f"{fn.__name__} {route} {shape} {str(dtype)[6:]} S={S} {name}", out[2] if compress else out)
                assert bool(status.all()), f"{fn.__name__} {name}: a member failed"
                factor = s32 if kw.get("scale") == third else 1.0
                for a, t in zip(accs, total):
                    assert torch.equal(a, t.float() * factor), f"{fn.__name__} {name}: wrong sum"
                if "out_nonfinite" in extra:
                    assert int(extra["out_nonfinite"].sum()) == 0, f"{fn.__name__} {name}: non-finite words counted"

    for route, torch_route in (("ctypes", False), ("torch", True)):
        dg.ops.prefer_torch_ops(torch_route)
        for dtype in (torch.bfloat16, torch.float16, torch.float32):
            for shape, words in REDUCE_SHAPES.items():
                if shape == "b65" and dtype == torch.float32:
                    continue
                ts, rows = sources(dtype, words, 10)
                n = len(words)
                if shape != "b65":
                    accs = [torch.ones([w], dtype=torch.float32, device=dev) for w in words]
                    used(f"decompress_accumulate {route} {shape}", dg.decompress_data_accumulate(rows[0], accs, True, prob_bits=10, dtype=dtype))
                    assert all(torch.equal(a, t.float() + 1) for a, t in zip(accs, ts[0])), "decode-accumulate mismatch"
                    for scale in (0.5, torch.full([1], 0.5, device=dev), torch.full([n], 0.5, device=dev)):
                        outs = [torch.empty([w], dtype=dtype, device=dev) for w in words]
                        used(f"decompress_scaled {route} {shape}", dg.decompress_data_scaled(rows[0], outs, scale, prob_bits=10))
                        assert all(torch.equal(o, t * 0.5) for o, t in zip(outs, ts[0])), "scaled decompress mismatch"
                    reduce_calls(route, dtype, shape, ts, rows, 10, False)
                if dtype != torch.float32:
                    reduce_calls(route, dtype, shape, ts, rows, 10, True)
        ts, rows = sources(torch.bfloat16, REDUCE_SHAPES["4block"], 11)
        for compress in (False, True):
            reduce_calls(route, torch.bfloat16, "4block", ts, rows, 11, compress)
    dg.ops.prefer_torch_ops(False)


def stochastic_compress(dg, torch, tensors, rows_of):
    """Stochastic cast-compress on both routes, after everything else (the lines of the calls above do not move, and the
    call reports no temp bytes): the shapes of the cast-compress calls, bf16 and fp16, a host seed and a device seed.  The
    archives decode to the words dietgpu_amd.rounding gives."""
    from dietgpu_amd import rounding

    dev = torch.device("cuda:0")
    held = torch.tensor([11], dtype=torch.int64, device=dev)
    for route in (False, True):
        dg.ops.prefer_torch_ops(route)
        for dtype in (torch.bfloat16, torch.float16):
            for words in ([100000] * 16, [64 * 1024 + 15000 * i for i in range(64)], [2 * 1024 * 1024] + [1000 + 37 * i for i in range(300)]):
                ts = tensors(torch.float32, words)
                for seed in (11, held):
                    comp, sizes = dg.compress_data_stochastic(ts, dtype, seed, 5, prob_bits=10)
                outs = [torch.empty([n], dtype=dtype, device=dev) for n in words]
                dg.decompress_data(True, rows_of(comp, sizes), outs, False, prob_bits=10)
                for i in (0, len(ts) - 1):
                    want = rounding.stochastic_round_(torch.empty_like(outs[i]), ts[i], 11, 5 + i)
                    assert torch.equal(outs[i].view(torch.int16), want.view(torch.int16)), "stochastic cast-compress mismatch"
    dg.ops.prefer_torch_ops(False)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--digest", default=None, help="the profiler's results database of a run of this script")
    ap.add_argument("--lines", default=None, help="with --digest: write the launch lines (and the tempUsed lines) here")
    ap.add_argument("--temp", default=None, help="with --digest: the --temp-out file of that run, which the digest then covers")
    ap.add_argument("--temp-out", default=None, help="write the tempUsed of every call here")
    a = ap.parse_args()
    if a.digest:
        digest(a.digest, a.lines, a.temp)
    else:
        main(a.temp_out)
