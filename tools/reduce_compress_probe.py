"""Reduce-compress against the two calls it replaces: 32 x 512 Ki bf16 accumulators, S archives each, P 10, on cache-cold
rotating buffer sets as bench.py's headline loop.  Two paths, interleaved, for S in 2, 4, 8:

  (a) decompress_data_reduce(..., accumulate=False) followed by compress_data_cast of the accumulators, as
      compressed_all_reduce made them before there was a reduce-compress;
  (b) one decompress_data_reduce_compress(..., accumulate=False).

Both leave the same bits, accumulators and archives (asserted first).  Then the kernels alone, HIP events around every
launch: k_ans_decode_reduce against k_ans_decode_reduce_stats, k_float_histogram_cast (path (a) only), k_normalize
(path (b) only: in (a) it runs inside the histogram kernel) and k_ans_encode_cast in both.  Prints one text report (the
figures of DESIGN.md section 5, profiles/reduce_compress_bf16_32x512Ki.txt).

Every S runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing
more is started.

    python tools/reduce_compress_probe.py [--steps 50] [--warmup 5] [--sets 4] [--limit 240]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(a, S):
    import torch

    sys.path.insert(0, ROOT)
    import dietgpu_amd as dg

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n = a.batch, a.words
    gen = torch.Generator(device="cpu").manual_seed(4321)
    cols = dg.max_float_compressed_size(torch.empty(0, dtype=torch.bfloat16), n)
    sets = []
    for _ in range(a.sets):
        archs, nbytes = [], 0  # [source][member]
        for _s in range(S):
            x = torch.randn((B, n), generator=gen).to(torch.bfloat16).to(dev)
            comp, sizes, _ = dg.compress_data(True, [x[i] for i in range(B)])
            archs.append([comp[i, :k] for i, k in enumerate(sizes.tolist())])  # rows of one matrix: 16-byte aligned
            nbytes += int(sizes.sum())
        acc = torch.zeros((B, n), dtype=torch.float32, device=dev)
        sets.append({"per_acc": [[archs[s][i] for s in range(S)] for i in range(B)], "acc": acc, "acc_rows": [acc[i] for i in range(B)],
                     "bytes": nbytes, "out": torch.empty((B, cols), dtype=torch.uint8, device=dev),
                     "out_sizes": torch.empty((B,), dtype=torch.int32, device=dev)})
    status = torch.zeros((B,), dtype=torch.uint8, device=dev)
    temp = torch.empty((dg.lib().dgpu_float_reduce_compress_temp_bytes(2, B, n),), dtype=torch.uint8, device=dev)

    def two_calls(st):
        dg.decompress_data_reduce(st["per_acc"], st["acc_rows"], False, temp, status, None, dtype=torch.bfloat16)
        dg.compress_data_cast(st["acc_rows"], torch.bfloat16, temp, st["out"], st["out_sizes"])

    def one_call(st):
        dg.decompress_data_reduce_compress(st["per_acc"], st["acc_rows"], False, temp, status, None, st["out"], st["out_sizes"],
                                           dtype=torch.bfloat16)

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
        return e0.elapsed_time(e1) / a.steps * 1000.0  # us per step

    # bit-exact first: accumulators, archive sizes, archive bytes up to the size
    archive_bytes = 0
    for st in sets:
        two_calls(st)
        assert bool(status.all())
        want_acc, want_sizes = st["acc"].clone(), st["out_sizes"].clone()
        want = [st["out"][i, :k].clone() for i, k in enumerate(want_sizes.tolist())]
        st["acc"].fill_(float("nan"))
        st["out"].fill_(0)
        one_call(st)
        assert bool(status.all()) and torch.equal(st["acc"].view(torch.int32), want_acc.view(torch.int32)), f"S={S}: accumulators"
        assert torch.equal(st["out_sizes"], want_sizes), f"S={S}: archive sizes"
        assert all(torch.equal(st["out"][i, : w.numel()], w) for i, w in enumerate(want)), f"S={S}: archive bytes"
        archive_bytes += int(want_sizes.sum())
    rows = [(timed(two_calls), timed(one_call)) for _ in range(3)]  # interleaved
    med = [sorted(r[i] for r in rows)[1] for i in range(2)]
    runs = lambda i: ", ".join("%.1f" % r[i] for r in rows)  # noqa: E731
    # the library's kernels alone: HIP events around every launch, a pass of its own over the same rotation
    L = dg.lib()
    L.dgpu_prof_reset()
    L.dgpu_prof_enable(1)
    for k in range(a.steps):
        two_calls(sets[k % a.sets])
        one_call(sets[k % a.sets])
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    L.dgpu_prof_summary(buf, len(buf))
    L.dgpu_prof_enable(0)
    prof = json.loads(buf.value.decode())
    kern = {k: (v["total_ms"] / v["launches"] * 1000.0, v["launches"]) for k, v in prof.items() if v.get("launches")}
    words = B * n
    comp = sum(st["bytes"] for st in sets) / len(sets)
    arch = archive_bytes / len(sets)
    traffic_b = comp + 4 * words + 4 * words + arch  # sources in, sums out, sums in once, archives out
    traffic_a = traffic_b + 4 * words                # ... and the sums in a second time, for the histogram
    print(f"  S = {S}: (a) {med[0]:8.1f} us per step (runs: {runs(0)})   (b) {med[1]:8.1f} us (runs: {runs(1)})   "
          f"(b) / (a) = {med[1] / med[0]:.3f}")
    names = ("k_ans_decode_reduce", "k_ans_decode_reduce_stats", "k_float_histogram_cast", "k_normalize", "k_ans_encode_cast")
    print("         kernels alone (events around each launch, the two paths alternating): " +
          ", ".join(f"{k} {kern[k][0]:.1f} us x {kern[k][1] // a.steps}" for k in names if k in kern))
    print(f"         algorithmic bytes per step: (a) at least {traffic_a / 1e6:.0f} MB, (b) at least {traffic_b / 1e6:.0f} MB "
          f"(if every round trip between sources is served from cache); (b) -> {traffic_b / med[1] / 1e6:.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--words", type=int, default=512 * 1024)
    ap.add_argument("--sources", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--limit", type=int, default=240, help="seconds every S may take")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        measure(a, a.child)
        return 0
    print(f"reduce-compress probe: {a.batch} x {a.words} bf16, P 10, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}, "
          f"median of 3 interleaved runs; (a) decompress_data_reduce + compress_data_cast, (b) one decompress_data_reduce_compress",
          flush=True)
    for S in a.sources:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(S), "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--sets", str(a.sets), "--batch", str(a.batch), "--words", str(a.words)]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"  S = {S}: no result within {a.limit} s; nothing more is started", flush=True)
            return 124
        if rc != 0:
            print(f"  S = {S}: ended with status {rc}; nothing more is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
