"""Rolling-table compress against the plain calls: 256 x 512 Ki bf16 and fp16, P 10, on cache-cold rotating buffer sets
as bench.py's headline loop.  Interleaved in one process:

  (a) compress_data (dgpu_float_compress): histogram pass + encoder -- the yardstick;
  (b) compress_data_rolling in steady state: counts_in = counts_out = one buffer per set, no histogram pass, the
      counting encoder;
  (c) compress_data_rolling with counts_out only: histogram pass + counting encoder (what the counting costs);
  (d) compress_data_cast against (e) its rolling form in steady state (float32 sources);
and the archive size of rolling against plain for a stream of tensors whose scale drifts 1 % per step, and for one whose
scale jumps 3 x up and down (the table of every step is the one the step before it left).

Prints one text report (the figures of DESIGN.md section 5, profiles/rolling_compress_256x512Ki.txt).

    python tools/rolling_compress_probe.py [--steps 100] [--warmup 10] [--sets 4]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dietgpu_amd as dg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--words", type=int, default=512 * 1024)
    ap.add_argument("--drift-steps", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n = a.batch, a.words
    gen = torch.Generator(device="cpu").manual_seed(1234)
    temp = torch.empty((int(dg.lib().dgpu_float_compress_temp_bytes(2, B, n)),), dtype=torch.uint8, device=dev)

    def timed(fn, sets):
        for k in range(a.warmup):
            fn(sets[k % len(sets)])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.steps):
            fn(sets[k % len(sets)])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps * 1000.0  # us per call

    print(f"rolling-compress probe: {B} x {n}, P 10, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}, "
          f"median of 3 interleaved runs")
    for dtype in (torch.bfloat16, torch.float16):
        cap = dg.max_float_compressed_size(torch.empty(0, dtype=dtype), n)
        sets = []
        for _ in range(a.sets):
            x32 = torch.randn((B, n), generator=gen).to(dev)
            x = x32.to(dtype)
            sets.append({"rows": [x[i] for i in range(B)], "rows32": [x32[i] for i in range(B)], "x": x, "x32": x32,
                         "comp": torch.empty((B, cap), dtype=torch.uint8, device=dev),
                         "sizes": torch.empty((B,), dtype=torch.int32, device=dev),
                         "counts": torch.empty((B, 256), dtype=torch.int32, device=dev),
                         "counts32": torch.empty((B, 256), dtype=torch.int32, device=dev)})

        def plain(s):
            dg.compress_data(True, s["rows"], False, temp, s["comp"], s["sizes"])

        def rolling(s):
            dg.compress_data_rolling(s["rows"], s["counts"], s["counts"], None, temp, s["comp"], s["sizes"])

        def counting(s):
            dg.compress_data_rolling(s["rows"], None, s["counts"], None, temp, s["comp"], s["sizes"])

        def cast_plain(s):
            dg.compress_data_cast(s["rows32"], dtype, temp, s["comp"], s["sizes"])

        def cast_rolling(s):
            dg.compress_data_rolling(s["rows32"], s["counts32"], s["counts32"], dtype, temp, s["comp"], s["sizes"])

        # byte-exact first: the counting call writes the plain archive (and leaves the counts the steady state starts from)
        for s in sets:
            plain(s)
            want, want_sizes = s["comp"].clone(), s["sizes"].clone()
            counting(s)
            mask = torch.arange(cap, device=dev)[None, :] < want_sizes[:, None]
            assert torch.equal(want_sizes, s["sizes"]) and torch.equal(torch.where(mask, want, 0), torch.where(mask, s["comp"], 0))
            dg.compress_data_rolling(s["rows32"], None, s["counts32"], dtype, temp, s["comp"], s["sizes"])
        fns = (plain, rolling, counting, cast_plain, cast_rolling)
        runs = [[timed(f, sets) for f in fns] for _ in range(3)]  # interleaved
        med = [sorted(r[i] for r in runs)[1] for i in range(len(fns))]
        show = lambda i: ", ".join("%.1f" % r[i] for r in runs)  # noqa: E731
        name = str(dtype).replace("torch.", "")
        print(f"{name}:")
        print(f"  (a) compress_data                                   {med[0]:8.1f} us per call   (runs: {show(0)})")
        print(f"  (b) compress_data_rolling, counts in = out          {med[1]:8.1f} us per call   (runs: {show(1)})   (b) / (a) = {med[1] / med[0]:.3f}")
        print(f"  (c) compress_data_rolling, counts out only          {med[2]:8.1f} us per call   (runs: {show(2)})   (c) / (a) = {med[2] / med[0]:.3f}")
        print(f"  (d) compress_data_cast (float32 source)             {med[3]:8.1f} us per call   (runs: {show(3)})")
        print(f"  (e) compress_data_rolling, float32 source, in = out {med[4]:8.1f} us per call   (runs: {show(4)})   (e) / (d) = {med[4] / med[3]:.3f}")

        # archive size of a stream: the table of step t is the one step t - 1 left
        def stream(scales, label):
            s = sets[0]
            first = s["x32"].to(dtype)
            dg.compress_data_rolling([first[i] for i in range(B)], None, s["counts"], None, temp, s["comp"], s["sizes"])
            ratios = []
            for step, scale in enumerate(scales, 1):
                cur = (sets[step % len(sets)]["x32"] * scale).to(dtype)  # another sample of the distribution, scaled
                rows = [cur[i] for i in range(B)]
                dg.compress_data(True, rows, False, temp, s["comp"], s["sizes"])
                own = int(s["sizes"].sum())
                dg.compress_data_rolling(rows, s["counts"], s["counts"], None, temp, s["comp"], s["sizes"])
                ratios.append(int(s["sizes"].sum()) / own)
            print(f"  archive bytes, rolling / plain, {label}: " + ", ".join("%.4f" % r for r in ratios))

        stream([1.01 ** k for k in range(1, a.drift_steps + 1)], "scale drifting 1 % per step")
        stream([3.0 if k % 2 else 1.0 for k in range(1, a.drift_steps + 1)], "scale jumping 3 x up, then 3 x down, ...")
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
