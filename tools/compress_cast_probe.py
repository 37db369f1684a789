"""Cast-compress against cast + compress: 256 x 512 Ki float32 -> bf16 archives, P 10, on cache-cold rotating buffer sets
as bench.py's headline loop.  Two paths, interleaved:

  (a) the path without the feature: x.to(torch.bfloat16) into a scratch matrix (ONE cast over all members), then
      compress_data of its rows;
  (b) one compress_data_cast.

Prints one text report (the figures of DESIGN.md section 5, profiles/compress_cast_bf16_256x512Ki.txt).

    python tools/compress_cast_probe.py [--steps 100] [--warmup 10] [--sets 4]
"""
import argparse
import ctypes
import json
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
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n = a.batch, a.words
    gen = torch.Generator(device="cpu").manual_seed(1234)
    cap = dg.max_float_compressed_size(torch.empty(0, dtype=torch.bfloat16), n)
    sets = []
    for _ in range(a.sets):
        x = torch.randn((B, n), generator=gen).to(dev)
        scratch = torch.empty((B, n), dtype=torch.bfloat16, device=dev)
        sets.append({"x": x, "rows": [x[i] for i in range(B)], "scratch": scratch, "scratch_rows": [scratch[i] for i in range(B)],
                     "comp": torch.empty((B, cap), dtype=torch.uint8, device=dev),
                     "sizes": torch.empty((B,), dtype=torch.int32, device=dev)})
    temp = torch.empty((int(dg.lib().dgpu_float_compress_temp_bytes(2, B, n)),), dtype=torch.uint8, device=dev)

    def cast_only(s):
        s["scratch"].copy_(s["x"])  # the cast kernel of x.to(torch.bfloat16), into a scratch that exists already

    def compress_only(s):
        dg.compress_data(True, s["scratch_rows"], False, temp, s["comp"], s["sizes"])

    def cast_then_compress(s):
        cast_only(s)
        compress_only(s)

    def compress_cast(s):
        dg.compress_data_cast(s["rows"], torch.bfloat16, temp, s["comp"], s["sizes"])

    def timed(fn):
        for k in range(a.warmup):
            fn(sets[k % a.sets])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.steps):
            fn(sets[k % a.sets])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps * 1000.0  # us per call

    # byte-exact first: both paths write the same archives (N(0, 1): no NaN, where torch's cast has other rules)
    comp_bytes = 0
    for s in sets:
        compress_cast(s)
        got, got_sizes = s["comp"].clone(), s["sizes"].clone()
        cast_then_compress(s)
        assert torch.equal(got_sizes, s["sizes"])
        mask = torch.arange(cap, device=dev)[None, :] < s["sizes"][:, None]
        assert torch.equal(torch.where(mask, got, 0), torch.where(mask, s["comp"], 0)), "the two paths wrote different archives"
        comp_bytes += int(s["sizes"].sum())
    comp_bytes /= len(sets)
    rows = []
    for rep in range(3):  # interleaved
        rows.append((timed(cast_then_compress), timed(compress_cast), timed(cast_only), timed(compress_only)))
    # the library's kernels alone: HIP events around every launch (dgpu_prof_*), a pass of its own over the same rotation
    L = dg.lib()
    L.dgpu_prof_reset()
    L.dgpu_prof_enable(1)
    for k in range(a.steps):
        cast_then_compress(sets[k % a.sets])
        compress_cast(sets[k % a.sets])
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    L.dgpu_prof_summary(buf, len(buf))
    L.dgpu_prof_enable(0)
    prof = json.loads(buf.value.decode())
    kern = {k: v["total_ms"] / v["launches"] * 1000.0 for k, v in prof.items() if v.get("launches")}
    med = [sorted(r[i] for r in rows)[1] for i in range(4)]
    words = B * n
    r_e = (comp_bytes - words) / words  # compressed bytes per word beyond the non-compressed byte (tables included)
    traffic_a = (4 + 2) * words + 2 * words + 2 * words + comp_bytes
    traffic_b = 4 * words + 4 * words + comp_bytes
    runs = lambda i: ", ".join("%.1f" % r[i] for r in rows)  # noqa: E731
    print(f"cast-compress probe: {B} x {n} float32 -> bf16, P 10, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}, "
          f"median of 3 interleaved runs")
    print(f"  (a) x.to(bfloat16) -> scratch, compress_data(scratch rows)   {med[0]:8.1f} us per step   (runs: {runs(0)})")
    print(f"  (b) compress_data_cast                                       {med[1]:8.1f} us per step   (runs: {runs(1)})")
    print(f"  (b) / (a) = {med[1] / med[0]:.3f}")
    print(f"  parts of (a), each in a loop of its own: cast {med[2]:.1f} us (runs: {runs(2)}), "
          f"compress_data {med[3]:.1f} us (runs: {runs(3)})")
    names = ("k_float_histogram", "k_ans_encode", "k_float_histogram_cast", "k_ans_encode_cast")
    if all(k in kern for k in names):
        print("  library kernels alone (events around each launch, (a) and (b) alternating): "
              + ", ".join(f"{k} {kern[k]:.1f} us" for k in names))
    print(f"  algorithmic bytes per step (r_e = {r_e:.3f}): (a) {traffic_a / 1e6:.0f} MB, (b) {traffic_b / 1e6:.0f} MB, "
          f"ratio {traffic_b / traffic_a:.3f}; at the measured times (a) moves {traffic_a / med[0] / 1e6:.2f} TB/s, "
          f"(b) {traffic_b / med[1] / 1e6:.2f} TB/s")


if __name__ == "__main__":
    main()
