"""What the squared norm and the non-finite count of a reduced shard cost: 32 x 512 Ki bf16 accumulators, S archives each,
P 10, summed into float32, scaled by 1/3 and compressed again on cache-cold rotating buffer sets as bench.py's headline
loop.  For S in 2, 4, 8:

  (a) decompress_data_reduce_compress(scale=1/3): the call of today;
  (b) the same call with out_sumsq / out_nonfinite: the statistic taken by the reduce kernel, per tile, when the tile's
      last source is stored;
  (c) (a) followed by what a training loop does today for clipping by global norm and for the overflow check of loss
      scaling: the accumulators cast to bf16 (the tensor every rank holds after the all-gather), torch.linalg.vector_norm
      of it in float64 and torch.isfinite(...).all().

(b)'s outputs are checked against (c)'s first, in every process: the same non-finite verdict, the squared norm within
n * 2**-52 of each other plus the float64 pass's own error.  Buffer placement alone moves these kernels by a few per cent
between processes (docs/HISTORY.md section 3), so every variant is measured in a fresh process of its own, twice: the
two runs of a variant are its A/A spread, the margin against which the ratios are read.  Every child process has its own
time limit.  Prints one text report (the figures of DESIGN.md section 5, profiles/reduce_norm_32x512Ki.txt).

    python tools/reduce_norm_probe.py [--runs 2] [--steps 40] [--warmup 5] [--sets 4] [--limit 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ("a", "b", "c")
SCALE = 1.0 / 3.0


def child(a):
    import torch

    import dietgpu_amd as dg

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n, smax = a.batch, a.words, max(a.sources)
    gen = torch.Generator(device="cpu").manual_seed(4321)
    sets = []
    for _ in range(a.sets):
        archs = []  # [source][member]
        for _s in range(smax):
            x = torch.randn((B, n), generator=gen).to(torch.bfloat16).to(dev)
            comp, sizes, _ = dg.compress_data(True, [x[i] for i in range(B)])
            archs.append([comp[i, :k] for i, k in enumerate(sizes.tolist())])  # rows of one matrix: 16-byte aligned
        acc = torch.zeros((B, n), dtype=torch.float32, device=dev)
        st = {"acc": acc, "acc_rows": [acc[i] for i in range(B)],
              "ins": {S: [[archs[s][i] for s in range(S)] for i in range(B)] for S in a.sources}}
        sets.append(st)
    status = torch.zeros((B,), dtype=torch.uint8, device=dev)
    cols = dg.max_float_compressed_size(torch.empty(0, dtype=torch.bfloat16), n)
    out_comp = torch.empty((B, cols), dtype=torch.uint8, device=dev)
    out_sizes = torch.empty((B,), dtype=torch.int32, device=dev)
    sumsq = torch.zeros((B,), dtype=torch.float64, device=dev)
    nonfinite = torch.zeros((B,), dtype=torch.int32, device=dev)
    temp = torch.empty((dg.lib().dgpu_float_reduce_norm_temp_bytes(2, B, n, 1),), dtype=torch.uint8, device=dev)
    seen = {}

    def run(st, S, v):
        if v == "b":
            dg.decompress_data_reduce_compress(st["ins"][S], st["acc_rows"], False, temp, status, None, out_comp, out_sizes, dtype=torch.bfloat16,
                                               scale=SCALE, out_sumsq=sumsq, out_nonfinite=nonfinite)
        else:
            dg.decompress_data_reduce_compress(st["ins"][S], st["acc_rows"], False, temp, status, None, out_comp, out_sizes, dtype=torch.bfloat16,
                                               scale=SCALE)
        if v == "c":
            cast = st["acc"].to(torch.bfloat16)
            seen["norm"] = torch.linalg.vector_norm(cast, dtype=torch.float64)
            seen["finite"] = torch.isfinite(cast).all()

    def timed(S, v):
        for k in range(a.warmup):
            run(sets[k % a.sets], S, v)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.steps):
            run(sets[k % a.sets], S, v)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps * 1000.0  # us per step

    # (b) says what (c) says
    for S in a.sources:
        st = sets[0]
        run(st, S, "c")
        assert bool(status.all()), S
        want_sq, want_finite = float(seen["norm"].item()) ** 2, bool(seen["finite"].item())
        archives = (out_sizes.clone(), out_comp.clone())
        st["acc"].fill_(float("nan"))
        run(st, S, "b")
        assert bool(status.all()), S
        got_sq, got_bad = float(sumsq.sum().item()), int(nonfinite.sum().item())
        assert (got_bad == 0) == want_finite, (S, got_bad, want_finite)
        assert abs(got_sq - want_sq) <= 4.0 * B * n * 2.0 ** -52 * want_sq, (S, got_sq, want_sq)
        assert torch.equal(out_sizes, archives[0]), S
        assert all(torch.equal(out_comp[i, :k], archives[1][i, :k]) for i, k in enumerate(out_sizes.tolist())), S
    res = {str(S): statistics.median(timed(S, a.variant) for _ in range(3)) for S in a.sources}
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--words", type=int, default=512 * 1024)
    ap.add_argument("--sources", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--variant", choices=VARIANTS)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    args = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup), "--sets", str(a.sets),
            "--batch", str(a.batch), "--words", str(a.words), "--sources"] + [str(s) for s in a.sources]
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
    print(f"reduce-norm probe: {a.batch} x {a.words} bf16, P 10, scale 1/3, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}; "
          f"per process the median of 3 runs, every variant in {a.runs} fresh processes of its own; us per step")
    print("  (a) reduce-compress   (b) reduce-compress with out_sumsq / out_nonfinite   (c) (a), then cast, vector_norm and isfinite().all()")
    for S in a.sources:
        per = {v: [r[str(S)] for r in runs[v]] for v in VARIANTS}
        mean = {v: statistics.mean(per[v]) for v in VARIANTS}
        spread = {v: (max(per[v]) - min(per[v])) / mean[v] for v in VARIANTS}
        cells = "   ".join(f"({v}) {mean[v]:7.1f} [{', '.join('%.1f' % x for x in per[v])}]" for v in VARIANTS)
        print(f"  S {S}: {cells}   b/a {mean['b'] / mean['a']:.3f} (+{mean['b'] - mean['a']:.1f} us)  b/c {mean['b'] / mean['c']:.3f}  "
              f"A/A spread (a) {100 * spread['a']:.1f} % (b) {100 * spread['b']:.1f} % (c) {100 * spread['c']:.1f} %")
    return 0


if __name__ == "__main__":
    sys.exit(main())
