"""Decode-reduce against the loop it replaces: 32 x 512 Ki bf16 accumulators, S archives each, P 10, summed into float32
on cache-cold rotating buffer sets as bench.py's headline loop.  Two paths, interleaved, for S in 2, 4, 8:

  (a) S successive decompress_data_accumulate calls (the first stores, the rest add), as compressed_reduce_scatter made
      them before there was a decode-reduce;
  (b) one decompress_data_reduce(..., accumulate=False).

Both leave the same bits (asserted first).  Prints one text report (the figures of DESIGN.md section 5,
profiles/decode_reduce_bf16_32x512Ki.txt).

    python tools/decode_reduce_probe.py [--steps 50] [--warmup 5] [--sets 4]
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--words", type=int, default=512 * 1024)
    ap.add_argument("--sources", type=int, nargs="+", default=[2, 4, 8])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n, smax = a.batch, a.words, max(a.sources)
    gen = torch.Generator(device="cpu").manual_seed(4321)
    sets = []
    for _ in range(a.sets):
        archs, nbytes = [], []  # [source][member]
        for _s in range(smax):
            x = torch.randn((B, n), generator=gen).to(torch.bfloat16).to(dev)
            comp, sizes, _ = dg.compress_data(True, [x[i] for i in range(B)])
            archs.append([comp[i, :k] for i, k in enumerate(sizes.tolist())])  # rows of one matrix: 16-byte aligned
            nbytes.append(int(sizes.sum()))
        acc = torch.zeros((B, n), dtype=torch.float32, device=dev)
        sets.append({"archs": archs, "acc": acc, "acc_rows": [acc[i] for i in range(B)], "bytes": nbytes})
    for st in sets:
        st["per_acc"] = {S: [[st["archs"][s][i] for s in range(S)] for i in range(B)] for S in a.sources}
    status = torch.zeros((B,), dtype=torch.uint8, device=dev)

    def loop_of_accumulates(st, S):
        for s in range(S):
            dg.decompress_data_accumulate(st["archs"][s], st["acc_rows"], s > 0, None, status, None, dtype=torch.bfloat16)

    def one_reduce(st, S):
        dg.decompress_data_reduce(st["per_acc"][S], st["acc_rows"], False, None, status, None, dtype=torch.bfloat16)

    def timed(fn, S):
        for k in range(a.warmup):
            fn(sets[k % a.sets], S)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.steps):
            fn(sets[k % a.sets], S)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps * 1000.0  # us per step

    # bit-exact first
    for S in a.sources:
        for st in sets:
            loop_of_accumulates(st, S)
            assert bool(status.all())
            want = st["acc"].clone()
            st["acc"].fill_(float("nan"))
            one_reduce(st, S)
            assert bool(status.all()) and torch.equal(st["acc"].view(torch.int32), want.view(torch.int32)), f"S={S}"
    print(f"decode-reduce probe: {B} x {n} bf16, P 10, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}, "
          f"median of 3 interleaved runs; (a) S decompress_data_accumulate calls, (b) one decompress_data_reduce")
    L = dg.lib()
    for S in a.sources:
        rows = [(timed(loop_of_accumulates, S), timed(one_reduce, S)) for _ in range(3)]  # interleaved
        med = [sorted(r[i] for r in rows)[1] for i in range(2)]
        runs = lambda i: ", ".join("%.1f" % r[i] for r in rows)  # noqa: E731
        # the library's kernels alone: HIP events around every launch, a pass of its own over the same rotation
        L.dgpu_prof_reset()
        L.dgpu_prof_enable(1)
        for k in range(a.steps):
            loop_of_accumulates(sets[k % a.sets], S)
            one_reduce(sets[k % a.sets], S)
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        L.dgpu_prof_summary(buf, len(buf))
        L.dgpu_prof_enable(0)
        prof = json.loads(buf.value.decode())
        kern = {k: v["total_ms"] / v["launches"] * 1000.0 for k, v in prof.items() if v.get("launches")}
        words = B * n
        comp = sum(sum(st["bytes"][:S]) for st in sets) / len(sets)
        traffic_a = comp + 4 * words * (2 * S - 1)  # a store, then S - 1 read-modify-write passes
        traffic_b = comp + 4 * words                # if every round trip between sources were served from cache
        print(f"  S = {S}: (a) {med[0]:8.1f} us per step (runs: {runs(0)})   (b) {med[1]:8.1f} us (runs: {runs(1)})   "
              f"(b) / (a) = {med[1] / med[0]:.3f}")
        ka, kr = kern.get("k_ans_decode_accum"), kern.get("k_ans_decode_reduce")
        if ka and kr:
            print(f"         kernels alone (events around each launch, alternating): k_ans_decode_accum {ka:.1f} us x {S}, "
                  f"k_ans_decode_reduce {kr:.1f} us")
        print(f"         algorithmic bytes per step: (a) {traffic_a / 1e6:.0f} MB -> {traffic_a / med[0] / 1e6:.2f} TB/s; (b) at least "
              f"{traffic_b / 1e6:.0f} MB, {traffic_a / 1e6:.0f} MB if no accumulator word stays in cache between sources")


if __name__ == "__main__":
    main()
