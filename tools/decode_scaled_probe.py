"""What a factor on the decode costs: 256 x 512 Ki bf16 (and fp16) archives, P 10, decoded on cache-cold rotating buffer
sets as bench.py's headline loop.

  (a) decompress_data: the plain decode;
  (b) decompress_data_scaled with a device factor of 1/3: the multiply in the decode kernel;
  (c) what a caller does without it: decompress_data, then mul_ of the decoded tensors by a 0-dim float32 factor -- a
      second pass that reads and writes 2 bytes per word;
  (d) decompress_data_scaled with a device factor of 1.0.

First, in every process: (b) and (c) leave the same bits at a factor that is exact in the type (0.5), and (b) at 1/3 and
(d) agree bit for bit with tests/scaled_ref.py on the first rows.  Buffer placement alone moves these kernels by a few
per cent between processes (docs/HISTORY.md section 3), so every variant is measured in a fresh process of its own,
twice: the two runs of a variant are its A/A spread, the margin against which the differences are read.  Every child
process has its own time limit.  Prints one text report (the figures of DESIGN.md section 5,
profiles/decode_scaled_256x512Ki.txt).

    python tools/decode_scaled_probe.py [--runs 2] [--steps 40] [--warmup 5] [--sets 4] [--limit 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("a", "b", "c", "d")
DTYPES = ("bfloat16", "float16")
SCALE = 1.0 / 3.0
CHECK_ROWS = 4  # rows compared with the host reference


def child(a):
    import numpy as np
    import torch

    import dietgpu_amd as dg

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scaled_ref as S

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n = a.batch, a.words
    res = {}
    for name in a.dtypes:
        dtype = getattr(torch, name)
        ft = S.BFLOAT16 if dtype == torch.bfloat16 else S.FLOAT16
        gen = torch.Generator(device=dev).manual_seed(4321)
        sets = []
        for _ in range(a.sets):
            x = torch.randn((B, n), generator=gen, device=dev).to(dtype)
            comp, sizes, _ = dg.compress_data(True, [x[i] for i in range(B)])
            rows = [comp[i, :k] for i, k in enumerate(sizes.tolist())]  # rows of one matrix: 16-byte aligned
            out = torch.empty((B, n), dtype=dtype, device=dev)
            sets.append({"x": x if not sets else None, "rows": rows, "out": out, "outs": [out[i] for i in range(B)]})
            del comp
        status = torch.zeros((B,), dtype=torch.uint8, device=dev)
        third = torch.tensor(SCALE, dtype=torch.float32, device=dev)
        one = torch.tensor(1.0, dtype=torch.float32, device=dev)
        half = torch.tensor(0.5, dtype=torch.float32, device=dev)

        def run(st, v, factor=None):
            if v == "a":
                dg.decompress_data(True, st["rows"], st["outs"], False, None, status, None)
            elif v == "c":
                dg.decompress_data(True, st["rows"], st["outs"], False, None, status, None)
                st["out"].mul_(third if factor is None else factor)
            else:
                dg.decompress_data_scaled(st["rows"], st["outs"], factor if factor is not None else (third if v == "b" else one), None, status, None)

        # (b) and (c) leave the same bits at a factor that is exact in the type; (b) and (d) against the host reference
        st = sets[0]
        words = lambda t: t[:CHECK_ROWS].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        src = words(st["x"])
        run(st, "b", half)
        assert bool(status.all())
        got_b = st["out"].view(torch.int16).clone()
        run(st, "c", half)
        assert torch.equal(st["out"].view(torch.int16), got_b), f"{name}: (b) and (c) differ at a factor of 0.5"
        for v, f in (("b", SCALE), ("d", 1.0)):
            st["out"].fill_(float("nan"))
            run(st, v)
            assert bool(status.all())
            assert np.array_equal(words(st["out"]), S.scaled_ref(src, ft, np.float32(f))), f"{name}: ({v}) differs from the reference"
        if a.variant == "d":
            assert torch.equal(st["out"].view(torch.int16), st["x"].view(torch.int16)), f"{name}: a factor of 1.0 changed a word"

        def timed(v):
            for k in range(a.warmup):
                run(sets[k % a.sets], v)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(a.steps):
                run(sets[k % a.sets], v)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.steps * 1000.0  # us per step

        res[name] = statistics.median(timed(a.variant) for _ in range(3))
        del sets
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--words", type=int, default=512 * 1024)
    ap.add_argument("--dtypes", nargs="+", default=list(DTYPES), choices=DTYPES)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--variant", choices=VARIANTS)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    args = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup), "--sets", str(a.sets),
            "--batch", str(a.batch), "--words", str(a.words), "--dtypes"] + list(a.dtypes)
    runs = {v: [] for v in VARIANTS}
    for _ in range(a.runs):
        for v in VARIANTS:  # a fresh process each: its own buffer placement, its own time limit
            try:
                p = subprocess.run(args + ["--variant", v], capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                sys.stderr.write(f"variant ({v}) did not finish within {a.limit} s\n")
                return 124
            if p.returncode != 0:  # nothing more is started after a child that failed
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                return p.returncode
            runs[v].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
            sys.stderr.write(f"({v}) {runs[v][-1]}\n")
    print(f"decode-scaled probe: {a.batch} x {a.words} words, P 10, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}; "
          f"per process the median of 3 runs, every variant in {a.runs} fresh processes of its own; us per step")
    print("  (a) decompress_data   (b) decompress_data_scaled, device factor 1/3   (c) decompress_data, mul_   (d) decompress_data_scaled, device factor 1.0")
    for name in a.dtypes:
        per = {v: [r[name] for r in runs[v]] for v in VARIANTS}
        mean = {v: statistics.mean(per[v]) for v in VARIANTS}
        spread = {v: (max(per[v]) - min(per[v])) / mean[v] for v in VARIANTS}
        cells = "   ".join(f"({v}) {mean[v]:7.1f} [{', '.join('%.1f' % x for x in per[v])}]" for v in VARIANTS)
        print(f"  {name}: {cells}")
        print(f"    b/a {mean['b'] / mean['a']:.3f}  d/a {mean['d'] / mean['a']:.3f}  b/c {mean['b'] / mean['c']:.3f}  "
              f"(c) - (b) {mean['c'] - mean['b']:.1f} us   A/A spread " + " ".join(f"({v}) {100 * spread[v]:.1f} %" for v in VARIANTS))
        verdict = mean["c"] - mean["b"] > max(spread["b"] * mean["b"], spread["c"] * mean["c"])
        print(f"    (b) below (c) by more than the larger of their A/A spreads: {'yes' if verdict else 'NO'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
