"""Feedback cast-compress against what it replaces: 256 x 512 Ki float32 -> bf16 and -> fp16 archives, P 10, on cache-cold
rotating buffer sets as bench.py's headline loop.  Three paths, each measured in a FRESH process of its own (one GPU step
= one child under its own time limit; the script stops at the first child that does not exit with 0):

  (a) compress_data_cast alone (no feedback: what the call costs without the residual);
  (b) compress_data_feedback, the residual updated in place;
  (c) the same step from existing calls: v = x + e, compress_data_cast(rows of v), e = v - v.to(dtype).float() with
      infinities and NaNs zeroed.

Every child also reports the library's kernels alone (dgpu_prof_summary: events around each launch).  The parent prints
one text report with the achieved fraction of the 8 TB/s HBM peak on the feedback form's algorithmic bytes: histogram 8
bytes read per word; encoder 8 read + 4 written per word, plus the archive.

    python tools/feedback_compress_probe.py [--steps 60] [--warmup 10] [--sets 4] [--timeout 240]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12  # bytes per second


def child(a):
    import torch

    sys.path.insert(0, ROOT)
    import dietgpu_amd as dg

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
        e = torch.zeros((B, n), device=dev)
        s = {"x": x, "e": e, "rows": [x[i] for i in range(B)], "erows": [e[i] for i in range(B)],
             "comp": torch.empty((B, cap), dtype=torch.uint8, device=dev), "sizes": torch.empty((B,), dtype=torch.int32, device=dev)}
        if a.path == "c":
            s["v"] = torch.empty((B, n), device=dev)
            s["vrows"] = [s["v"][i] for i in range(B)]
            s["w"] = torch.empty((B, n), device=dev)
        sets.append(s)
    temp = torch.empty((int(dg.lib().dgpu_float_compress_temp_bytes(ft, B, n)),), dtype=torch.uint8, device=dev)

    def cast(s):
        dg.compress_data_cast(s["rows"], dtype, temp, s["comp"], s["sizes"])

    def feedback(s):
        dg.compress_data_feedback(s["rows"], s["erows"], dtype, False, temp, s["comp"], s["sizes"])

    def unfused(s):
        torch.add(s["x"], s["e"], out=s["v"])
        dg.compress_data_cast(s["vrows"], dtype, temp, s["comp"], s["sizes"])
        s["w"].copy_(s["v"].to(dtype))                       # widen(q): the cast and its way back
        torch.sub(s["v"], s["w"], out=s["e"])
        s["e"].masked_fill_(~torch.isfinite(s["w"]), 0.0)    # zero where q is an infinity or a NaN

    fn = {"a": cast, "b": feedback, "c": unfused}[a.path]
    # (one first step from a zero residual, so that every measured step adds a residual of realistic size)
    for s in sets:
        (feedback if a.path != "c" else unfused)(s)

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
    ap.add_argument("--path", choices=["a", "b", "c"], help="(child) the path to measure")
    ap.add_argument("--dtype", choices=["bf16", "fp16"], help="(child) the archive type")
    a = ap.parse_args()
    if a.path:
        return child(a)
    words = a.batch * a.words
    print(f"feedback cast-compress probe: {a.batch} x {a.words} float32, P 10, {a.sets} rotating buffer sets, {a.steps} steps after "
          f"{a.warmup}, median of 3 runs, every path in a fresh process")
    for dtype in ("bf16", "fp16"):
        res = {}
        for path in ("a", "b", "c", "b", "a"):  # (a) and (b) twice, around (c): the spread between two processes shows
            cmd = [sys.executable, os.path.abspath(__file__), "--path", path, "--dtype", dtype] + [
                f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "sets", "batch", "words")]
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
        show = lambda k: " / ".join("%.1f" % m for m in med[k])  # noqa: E731
        print(f"-> {dtype}")
        print(f"  (a) compress_data_cast alone                       {show('a'):>16} us per step")
        print(f"  (b) compress_data_feedback, in place               {show('b'):>16} us per step")
        print(f"  (c) add, compress_data_cast, cast back, sub, mask  {show('c'):>16} us per step")
        b, c = min(med["b"]), min(med["c"])
        print(f"  (b) / (c) = {b / c:.3f}   (b) - (a) = {b - min(med['a']):.1f} us")
        for path in ("a", "b", "c"):
            k = res[path][0]["kernels"]
            print(f"  library kernels alone, path ({path}): " + ", ".join(f"{n} {t:.1f} us" for n, t in sorted(k.items())))
        comp = res["b"][0]["comp_bytes"]
        kb = res["b"][0]["kernels"]
        hist, enc = kb.get("k_float_histogram_feedback"), kb.get("k_ans_encode_feedback")
        if hist and enc:
            hb, eb = 8 * words, 12 * words + comp
            print(f"  algorithmic bytes of (b): histogram {hb / 1e6:.0f} MB, encoder {eb / 1e6:.0f} MB (archive {comp / 1e6:.0f} MB): "
                  f"histogram {hb / hist / 1e6:.2f} TB/s = {hb / hist * 1e6 / PEAK:.0%} of peak, encoder {eb / enc / 1e6:.2f} TB/s = "
                  f"{eb / enc * 1e6 / PEAK:.0%} of peak, the step {(hb + eb) / b / 1e6:.2f} TB/s = {(hb + eb) / b * 1e6 / PEAK:.0%}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
