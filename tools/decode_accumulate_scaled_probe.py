"""What float32 out of a 16-bit archive costs with a factor: 256 x 512 Ki bf16 (and fp16) archives, P 10, decoded into
float32 on cache-cold rotating buffer sets as bench.py's headline loop.

  (a) decompress_data_accumulate(accumulate=False): the floor -- 4 bytes written per word;
  (b) (a) with a device factor of 1/3: the multiply in the decode kernel;
  (c) (b) with accumulate=True: 4 bytes more read per word;
  (d) the composition (b) replaces: decode-accumulate into a float32 scratch, then mul_ by a 0-dim float32 factor;
  (e) the composition (c) replaces: (d), then add_ into the accumulator;
  (f) what a caller does today after the all-reduce: decompress_data_scaled into 16 bits, then .float().

First, in every process: (b) and (d), and (c) and (e), leave the same bits, and (b) agrees bit for bit with
tests/accum_scaled_ref.py on the first rows.  Buffer placement alone moves these kernels by a few per cent between
processes (docs/HISTORY.md section 3), so every variant is measured in a fresh process of its own, twice: the two runs
of a variant are its A/A spread, the margin against which the differences are read.  Every child process has its own
time limit.  Prints one text report (the figures of DESIGN.md section 5, profiles/decode_accumulate_scaled_256x512Ki.txt).

    python tools/decode_accumulate_scaled_probe.py [--runs 2] [--steps 40] [--warmup 5] [--sets 4] [--limit 240] [--variants a f]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("a", "b", "c", "d", "e", "f")
DTYPES = ("bfloat16", "float16")
SCALE = 1.0 / 3.0
CHECK_ROWS = 4  # rows compared with the host reference


def child(a):
    import numpy as np
    import torch

    import dietgpu_amd as dg

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import accum_scaled_ref as A

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n = a.batch, a.words
    res = {}
    for name in a.dtypes:
        dtype = getattr(torch, name)
        ft = A.BFLOAT16 if dtype == torch.bfloat16 else A.FLOAT16
        gen = torch.Generator(device=dev).manual_seed(4321)
        sets = []
        for _ in range(a.sets):
            x = torch.randn((B, n), generator=gen, device=dev).to(dtype)
            comp, sizes, _ = dg.compress_data(True, [x[i] for i in range(B)])
            rows = [comp[i, :k] for i, k in enumerate(sizes.tolist())]  # rows of one matrix: 16-byte aligned
            acc = torch.zeros((B, n), dtype=torch.float32, device=dev)
            sets.append({"x": x[:CHECK_ROWS].clone() if not sets else None, "rows": rows, "acc": acc, "accs": [acc[i] for i in range(B)]})
            del comp, x
        # one scratch for the compositions, as a caller would keep one; (f) decodes into a 16-bit one
        wide = torch.empty((B, n), dtype=torch.float32, device=dev) if a.variant in ("d", "e") or not a.timing_only else None
        wides = [wide[i] for i in range(B)] if wide is not None else None
        narrow = torch.empty((B, n), dtype=dtype, device=dev) if a.variant == "f" else None
        narrows = [narrow[i] for i in range(B)] if narrow is not None else None
        status = torch.zeros((B,), dtype=torch.uint8, device=dev)
        third = torch.tensor(SCALE, dtype=torch.float32, device=dev)

        def run(st, v):
            if v == "a":
                dg.decompress_data_accumulate(st["rows"], st["accs"], False, None, status, None, dtype=dtype)
            elif v == "b":
                dg.decompress_data_accumulate(st["rows"], st["accs"], False, None, status, None, dtype=dtype, scale=third)
            elif v == "c":
                dg.decompress_data_accumulate(st["rows"], st["accs"], True, None, status, None, dtype=dtype, scale=third)
            elif v in ("d", "e"):
                dg.decompress_data_accumulate(st["rows"], wides, False, None, status, None, dtype=dtype)
                wide.mul_(third)  # (d): the result stays in the scratch
                if v == "e":
                    st["acc"].add_(wide)
            else:
                dg.decompress_data_scaled(st["rows"], narrows, third, None, status, None)
                st["acc"].copy_(narrow)  # .float() into the float32 buffer

        if not a.timing_only:
            st = sets[0]
            bits = lambda t: t[:CHECK_ROWS].contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
            src = st["x"].view(torch.int16).cpu().numpy().view(np.uint16)
            st["acc"].fill_(float("nan"))
            run(st, "b")
            assert bool(status.all())
            got_b = st["acc"].view(torch.int32).clone()
            assert np.array_equal(bits(st["acc"]), A.accum_scaled_ref(src, ft, np.float32(SCALE))), f"{name}: (b) differs from the reference"
            run(st, "d")
            assert torch.equal(wide.view(torch.int32), got_b), f"{name}: (b) and (d) differ"
            st["acc"].fill_(1.25)
            run(st, "c")
            got_c = st["acc"].view(torch.int32).clone()
            st["acc"].fill_(1.25)
            run(st, "e")
            assert torch.equal(st["acc"].view(torch.int32), got_c), f"{name}: (c) and (e) differ"
            del got_b, got_c

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
        del sets, wide, wides, narrow, narrows
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
    ap.add_argument("--variants", nargs="+", default=list(VARIANTS), choices=VARIANTS, help="the legs to measure")
    ap.add_argument("--timing-only", action="store_true", help="skip the bit checks (a library without the scaled call: legs a and f)")
    ap.add_argument("--variant", choices=VARIANTS)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    args = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup), "--sets", str(a.sets),
            "--batch", str(a.batch), "--words", str(a.words)] + (["--timing-only"] if a.timing_only else []) + ["--dtypes"] + list(a.dtypes)
    legs = [v for v in VARIANTS if v in a.variants]
    runs = {v: [] for v in legs}
    for _ in range(a.runs):
        for v in legs:  # a fresh process each: its own buffer placement, its own time limit
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
    print(f"decode-accumulate-scaled probe: {a.batch} x {a.words} words, P 10, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}; "
          f"per process the median of 3 runs, every variant in {a.runs} fresh processes of its own; us per step")
    print("  (a) decompress_data_accumulate, store   (b) (a) with a device factor 1/3   (c) (b) with accumulate   "
          "(d) (a) into a scratch, mul_   (e) (d), add_   (f) decompress_data_scaled, .float()")
    for name in a.dtypes:
        per = {v: [r[name] for r in runs[v]] for v in legs}
        mean = {v: statistics.mean(per[v]) for v in legs}
        spread = {v: (max(per[v]) - min(per[v])) / mean[v] for v in legs}
        print(f"  {name}: " + "   ".join(f"({v}) {mean[v]:7.1f} [{', '.join('%.1f' % x for x in per[v])}]" for v in legs))
        print("    A/A spread " + " ".join(f"({v}) {100 * spread[v]:.1f} %" for v in legs))
        for lo, hi in (("b", "d"), ("b", "f"), ("c", "e")):
            if lo in mean and hi in mean:
                verdict = mean[hi] - mean[lo] > max(spread[lo] * mean[lo], spread[hi] * mean[hi])
                print(f"    ({lo}) below ({hi}) by more than the larger of their A/A spreads: {'yes' if verdict else 'NO'}  "
                      f"({lo})/({hi}) {mean[lo] / mean[hi]:.3f}, ({hi}) - ({lo}) {mean[hi] - mean[lo]:.1f} us")
        if "a" in mean and "b" in mean and "c" in mean:
            print(f"    b/a {mean['b'] / mean['a']:.3f}  c/a {mean['c'] / mean['a']:.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
