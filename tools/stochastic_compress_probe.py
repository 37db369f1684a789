"""Stochastic cast-compress against its alternatives: 256 x 512 Ki float32 -> bf16 and -> fp16 archives, P 10, on cache-cold
rotating buffer sets as bench.py's headline loop.  Four paths, each measured in a FRESH process of its own (one GPU step =
one child under its own time limit; the script stops at the first child that does not exit with 0), interleaved in one
command:

  (a) compress_data_stochastic (a host seed that changes every step);
  (b) compress_data_cast: round to nearest, the yardstick of the same run;
  (c) compress_data_feedback, the residual updated in place: the remedy the stochastic call replaces (4 B per element of
      residual, loaded and stored by both kernels);
  (d) the same archives from existing calls: rounding.stochastic_round_ into a 16-bit scratch, then compress_data.

Every child also reports the library's kernels alone (dgpu_prof_summary: events around each launch).

    python tools/stochastic_compress_probe.py [--steps 60] [--warmup 10] [--sets 4] [--timeout 240] [--paths a,b,c,d]
                                              [--route ops|ctypes]

--paths b,c --route ctypes with DGPU_LIB naming a library built from an earlier revision measures that build's (b) and (c)
on the same route (the op library links the tree's own core library, so an A/B goes through ctypes on both sides).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = {"a": "compress_data_stochastic", "b": "compress_data_cast (nearest)", "c": "compress_data_feedback, in place",
         "d": "stochastic_round_ + compress_data"}


def child(a):
    import torch

    sys.path.insert(0, ROOT)
    import dietgpu_amd as dg
    from dietgpu_amd import rounding

    dg.prefer_torch_ops(a.route == "ops")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype]
    ft = {"bf16": 2, "fp16": 1}[a.dtype]
    B, n = a.batch, a.words
    gen = torch.Generator(device="cpu").manual_seed(1234)
    cap = dg.max_float_compressed_size(torch.empty(0, dtype=dtype), n)
    sets = []
    for _ in range(a.sets):
        x = torch.randn((B, n), generator=gen).to(dev)
        s = {"x": x, "rows": [x[i] for i in range(B)], "comp": torch.empty((B, cap), dtype=torch.uint8, device=dev),
             "sizes": torch.empty((B,), dtype=torch.int32, device=dev)}
        if a.path == "c":
            s["e"] = torch.zeros((B, n), device=dev)
            s["erows"] = [s["e"][i] for i in range(B)]
        if a.path == "d":
            s["q"] = torch.empty((B, n), dtype=dtype, device=dev)
            s["qrows"] = [s["q"][i] for i in range(B)]
        sets.append(s)
    temp = torch.empty((int(dg.lib().dgpu_float_compress_temp_bytes(ft, B, n)),), dtype=torch.uint8, device=dev)
    step = [0]

    def stochastic(s):
        step[0] += 1
        dg.compress_data_stochastic(s["rows"], dtype, step[0], 0, s["comp"], s["sizes"])

    def cast(s):
        dg.compress_data_cast(s["rows"], dtype, temp, s["comp"], s["sizes"])

    def feedback(s):
        dg.compress_data_feedback(s["rows"], s["erows"], dtype, False, temp, s["comp"], s["sizes"])

    def unfused(s):
        step[0] += 1
        # (one member for the whole matrix: the bits differ from (a)'s, the work does not)
        rounding.stochastic_round_(s["q"], s["x"], step[0], 0)
        dg.compress_data(True, s["qrows"], False, temp, s["comp"], s["sizes"])

    fn = {"a": stochastic, "b": cast, "c": feedback, "d": unfused}[a.path]
    for s in sets:  # (c): one first step from a zero residual, so that every measured step adds a residual of realistic size
        fn(s)

    def timed():
        for k in range(a.warmup):
            fn(sets[k % a.sets])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.steps):
            fn(sets[k % a.sets])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps * 1000.0  # us per step

    runs = [timed() for _ in range(3)]
    comp_bytes = sum(int(s["sizes"].sum()) for s in sets) / len(sets)
    L = dg.lib()
    L.dgpu_prof_reset()
    L.dgpu_prof_enable(1)
    for k in range(a.steps):
        fn(sets[k % a.sets])
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    L.dgpu_prof_summary(buf, len(buf))
    L.dgpu_prof_enable(0)
    prof = json.loads(buf.value.decode())
    kern = {k: v["total_ms"] / v["launches"] * 1000.0 for k, v in prof.items() if v.get("launches")}
    print("RESULT " + json.dumps({"path": a.path, "dtype": a.dtype, "runs": runs, "comp_bytes": comp_bytes, "kernels": kern}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--words", type=int, default=512 * 1024)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--paths", default="a,b,c,d", help="the paths to measure, e.g. b,c")
    ap.add_argument("--route", choices=["ops", "ctypes"], default="ops", help="torch ops (the default route) or ctypes")
    ap.add_argument("--path", choices=["a", "b", "c", "d"], help="(child) the path to measure")
    ap.add_argument("--dtype", choices=["bf16", "fp16"], help="(child) the archive type")
    a = ap.parse_args()
    if a.path:
        return child(a)
    paths = [p for p in a.paths.split(",") if p]
    lib = os.environ.get("DGPU_LIB")
    print(f"stochastic cast-compress probe: {a.batch} x {a.words} float32, P 10, {a.sets} rotating buffer sets, {a.steps} steps after "
          f"{a.warmup}, median of 3 runs, every path in a fresh process, route {a.route}" + (f", library {os.path.basename(lib)}" if lib else ""))
    for dtype in ("bf16", "fp16"):
        res = {}
        for path in paths + paths[-2::-1]:  # there and back: every path but the last twice, the spread between two processes shows
            cmd = [sys.executable, os.path.abspath(__file__), "--path", path, "--dtype", dtype] + [
                f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "sets", "batch", "words", "route")]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"child {path} {dtype} ran into its time limit of {a.timeout} s; stopping")
                return 124
            if p.returncode != 0:
                print(f"child {path} {dtype} exited with {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
                return p.returncode
            line = next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))
            res.setdefault(path, []).append(json.loads(line[7:]))
        med = {k: [sorted(r["runs"])[1] for r in v] for k, v in res.items()}
        print(f"-> {dtype}")
        for path in paths:
            print(f"  ({path}) {LABEL[path]:<36} {' / '.join('%.1f' % m for m in med[path]):>16} us per step")
        if "a" in med and "b" in med:
            print(f"  (a) / (b) = {min(med['a']) / min(med['b']):.3f}   (a) - (b) = {min(med['a']) - min(med['b']):.1f} us")
        if "a" in med and "c" in med:
            print(f"  (a) / (c) = {min(med['a']) / min(med['c']):.3f}   (a) - (c) = {min(med['a']) - min(med['c']):.1f} us")
        if "a" in med and "d" in med:
            print(f"  (a) / (d) = {min(med['a']) / min(med['d']):.3f}")
        for path in paths:
            k = res[path][0]["kernels"]
            print(f"  library kernels alone, path ({path}): " + ", ".join(f"{n} {t:.1f} us" for n, t in sorted(k.items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
