"""Ranged decode against the whole decode: 256 x 512 Ki bf16, P 10, blocks [32, 48) of every element (one 16-block tile
of eight), on cache-cold rotating buffer sets as bench.py's headline loop.  Prints one text report (the figures of
DESIGN.md section 5, profiles/range_decode_bf16_256x512Ki.txt).

    python tools/range_decode_probe.py [--steps 200] [--warmup 20] [--sets 4] [--first 32] [--blocks 16]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dietgpu_amd as dg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--words", type=int, default=512 * 1024)
    ap.add_argument("--first", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=16)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n = a.batch, a.words
    gen = torch.Generator(device="cpu").manual_seed(1234)
    sets = []
    for _ in range(a.sets):
        x = torch.randn((B, n), generator=gen).to(torch.bfloat16).to(dev)
        xs = [x[i] for i in range(B)]
        comp, sizes, _ = dg.compress_data(True, xs)
        archs = [comp[i, :s] for i, s in enumerate(sizes.tolist())]  # rows of one matrix: 16-byte aligned
        full = torch.empty((B, n), dtype=torch.bfloat16, device=dev)
        part = torch.empty((B, a.blocks * 4096), dtype=torch.bfloat16, device=dev)
        sets.append((x, archs, [full[i] for i in range(B)], full, [part[i] for i in range(B)], part))
    status = torch.zeros((B,), dtype=torch.uint8, device=dev)
    temp = torch.empty((16 << 20,), dtype=torch.uint8, device=dev)
    first, count = [a.first] * B, [a.blocks] * B

    def whole(s):
        dg.decompress_data(True, s[1], s[2], False, temp, status, None)

    def ranged(s):
        dg.decompress_data_range(True, s[1], s[4], first, count, temp, status, None)

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

    # bit-exact first
    for s in sets:
        whole(s)
        assert bool(status.all()) and torch.equal(s[3].view(torch.int16), s[0].view(torch.int16))
        ranged(s)
        lo = a.first * 4096
        assert bool(status.all()) and torch.equal(s[5].view(torch.int16), s[0][:, lo : lo + a.blocks * 4096].view(torch.int16))
    rows = []
    for rep in range(3):  # interleaved
        rows.append((timed(whole), timed(ranged)))
    # the kernels alone: HIP events around every launch (dgpu_prof_*), a pass of its own over the same rotation
    import ctypes
    import json

    L = dg.lib()
    L.dgpu_prof_reset()
    L.dgpu_prof_enable(1)
    for k in range(a.steps):
        whole(sets[k % a.sets])
        ranged(sets[k % a.sets])
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    L.dgpu_prof_summary(buf, len(buf))
    L.dgpu_prof_enable(0)
    prof = json.loads(buf.value.decode())
    kern = {k: v["total_ms"] / v["launches"] * 1000.0 for k, v in prof.items() if v.get("launches")}
    w = sorted(r[0] for r in rows)[1]
    r = sorted(r[1] for r in rows)[1]
    print(f"ranged decode probe: {B} x {n} bf16, P 10, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}, median of 3 interleaved runs")
    print(f"  whole decode                      {w:8.1f} us per call   (runs: {', '.join('%.1f' % x[0] for x in rows)})")
    print(f"  blocks [{a.first}, {a.first + a.blocks}) of every element  {r:8.1f} us per call   (runs: {', '.join('%.1f' % x[1] for x in rows)})")
    print(f"  ranged / whole = {r / w:.3f}   (blocks decoded: {a.blocks} of {(n + 4095) // 4096} = {a.blocks * 4096 / n:.3f})")
    kw, kr = kern.get("k_ans_decode"), kern.get("k_ans_decode_range")
    if kw and kr:
        print(f"  kernels alone (events around each launch, whole and ranged alternating): k_ans_decode {kw:.1f} us, "
              f"k_ans_decode_range {kr:.1f} us, ratio {kr / kw:.3f}")
    print("  (a call = host work + launch; the ranged call goes through the pointer-array path and its parameter cache,")
    print("   the whole decode of the rows of one matrix is a stride batch: when the loop is host-bound the call time is the host's)")


if __name__ == "__main__":
    main()
