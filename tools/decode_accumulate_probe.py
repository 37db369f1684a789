"""Decode-accumulate against decode + add: 256 x 512 Ki bf16 archives, P 10, summed into float32 accumulators, on
cache-cold rotating buffer sets as bench.py's headline loop.  Two paths, interleaved:

  (a) the path without the feature: decompress_data into a bf16 scratch matrix, then acc.add_(scratch) -- ONE add over
      all members (the cheapest form of "an add for every member": one launch instead of 256);
  (b) one decompress_data_accumulate(..., accumulate=True).

Prints one text report (the figures of DESIGN.md section 5, profiles/decode_accumulate_bf16_256x512Ki.txt).

    python tools/decode_accumulate_probe.py [--steps 100] [--warmup 10] [--sets 4]
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
    sets = []
    for _ in range(a.sets):
        x = torch.randn((B, n), generator=gen).to(torch.bfloat16).to(dev)
        comp, sizes, _ = dg.compress_data(True, [x[i] for i in range(B)])
        archs = [comp[i, :s] for i, s in enumerate(sizes.tolist())]  # rows of one matrix: 16-byte aligned
        scratch = torch.empty((B, n), dtype=torch.bfloat16, device=dev)
        acc = torch.zeros((B, n), dtype=torch.float32, device=dev)
        sets.append({"x": x, "archs": archs, "scratch": scratch, "scratch_rows": [scratch[i] for i in range(B)], "acc": acc,
                     "acc_rows": [acc[i] for i in range(B)], "bytes": int(sizes.sum())})
    status = torch.zeros((B,), dtype=torch.uint8, device=dev)
    temp = torch.empty((16 << 20,), dtype=torch.uint8, device=dev)

    def decode_then_add(s):
        dg.decompress_data(True, s["archs"], s["scratch_rows"], False, temp, status, None)
        s["acc"].add_(s["scratch"])

    def decode_only(s):
        dg.decompress_data(True, s["archs"], s["scratch_rows"], False, temp, status, None)

    def add_only(s):
        s["acc"].add_(s["scratch"])

    def decode_accumulate(s):
        dg.decompress_data_accumulate(s["archs"], s["acc_rows"], True, temp, status, None, dtype=torch.bfloat16)

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

    # bit-exact first: both paths give acc + float32(x), twice in a row
    for s in sets:
        want = s["x"].to(torch.float32)
        decode_accumulate(s)
        assert bool(status.all()) and torch.equal(s["acc"].view(torch.int32), want.view(torch.int32))
        decode_then_add(s)
        assert bool(status.all()) and torch.equal(s["acc"].view(torch.int32), (want + want).view(torch.int32))
        s["acc"].zero_()
    rows = []
    for rep in range(3):  # interleaved
        rows.append((timed(decode_then_add), timed(decode_accumulate), timed(decode_only), timed(add_only)))
        for s in sets:
            s["acc"].zero_()  # (sums of N(0,1) stay far from overflow anyway)
    # the library's kernels alone: HIP events around every launch (dgpu_prof_*), a pass of its own over the same rotation
    L = dg.lib()
    L.dgpu_prof_reset()
    L.dgpu_prof_enable(1)
    for k in range(a.steps):
        decode_then_add(sets[k % a.sets])
        decode_accumulate(sets[k % a.sets])
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    L.dgpu_prof_summary(buf, len(buf))
    L.dgpu_prof_enable(0)
    prof = json.loads(buf.value.decode())
    kern = {k: v["total_ms"] / v["launches"] * 1000.0 for k, v in prof.items() if v.get("launches")}
    med = [sorted(r[i] for r in rows)[1] for i in range(4)]
    words = B * n
    comp_bytes = sum(s["bytes"] for s in sets) / len(sets)
    traffic_a = comp_bytes + 2 * words + 2 * words + 4 * words + 4 * words
    traffic_b = comp_bytes + 4 * words + 4 * words
    runs = lambda i: ", ".join("%.1f" % r[i] for r in rows)  # noqa: E731
    print(f"decode-accumulate probe: {B} x {n} bf16, P 10, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}, "
          f"median of 3 interleaved runs")
    print(f"  (a) decompress_data -> bf16 scratch, acc.add_(scratch)   {med[0]:8.1f} us per step   (runs: {runs(0)})")
    print(f"  (b) decompress_data_accumulate(accumulate=True)          {med[1]:8.1f} us per step   (runs: {runs(1)})")
    print(f"  (b) / (a) = {med[1] / med[0]:.3f}")
    print(f"  parts of (a), each in a loop of its own: decompress_data {med[2]:.1f} us (runs: {runs(2)}), "
          f"acc.add_ {med[3]:.1f} us (runs: {runs(3)})")
    kd, ka = kern.get("k_ans_decode"), kern.get("k_ans_decode_accum")
    if kd and ka:
        print(f"  library kernels alone (events around each launch, (a) and (b) alternating): k_ans_decode {kd:.1f} us, "
              f"k_ans_decode_accum {ka:.1f} us")
    print(f"  algorithmic bytes per step: (a) {traffic_a / 1e6:.0f} MB, (b) {traffic_b / 1e6:.0f} MB, ratio {traffic_b / traffic_a:.3f}; "
          f"at the measured times (a) moves {traffic_a / med[0] / 1e6:.2f} TB/s, (b) {traffic_b / med[1] / 1e6:.2f} TB/s")


if __name__ == "__main__":
    main()
