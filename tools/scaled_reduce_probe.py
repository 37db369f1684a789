"""What a mean costs: 32 x 512 Ki bf16 accumulators, S archives each, P 10, summed into float32 and compressed again on
cache-cold rotating buffer sets as bench.py's headline loop.  For S in 2, 4, 8:

  (a) decompress_data_reduce_compress, unscaled: the sum;
  (b) decompress_data_reduce_compress(scale=1/3): the scaled sum, the multiply in the reduce kernel;
  (c) what a scaled sum costs without it: decompress_data_reduce, mul_ of the float32 accumulators by a float32 scalar,
      compress_data_cast -- 12 more bytes per word through HBM than (b): the mul_ reads and writes the accumulators
      (8), and the cast's histogram pass reads them once more (4).

(b) and (c) leave the same accumulators and archives (asserted first, in every process).  Buffer placement alone moves
these kernels by a few per cent between processes (docs/HISTORY.md section 3), so every variant is measured in a fresh
process of its own, twice: the two runs of a variant are its A/A spread, the margin against which the ratios are read.
Every child process has its own time limit.  Prints one text report (the figures of DESIGN.md section 5,
profiles/scaled_reduce_32x512Ki.txt).

    python tools/scaled_reduce_probe.py [--runs 2] [--steps 40] [--warmup 5] [--sets 4] [--limit 240]
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
    factor = torch.tensor(SCALE, dtype=torch.float32, device=dev)

    def run(st, S, v):
        if v == "c":
            dg.decompress_data_reduce(st["ins"][S], st["acc_rows"], False, None, status, None, dtype=torch.bfloat16)
            st["acc"].mul_(factor)
            dg.compress_data_cast(st["acc_rows"], torch.bfloat16, None, out_comp, out_sizes)
        else:
            dg.decompress_data_reduce_compress(st["ins"][S], st["acc_rows"], False, None, status, None, out_comp, out_sizes, dtype=torch.bfloat16,
                                               scale=SCALE if v == "b" else None)

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

    # (b) and (c) leave the same bits
    for S in a.sources:
        st = sets[0]
        want = None
        for v in ("b", "c"):
            st["acc"].fill_(float("nan"))
            run(st, S, v)
            assert bool(status.all()), (S, v)
            got = (st["acc"].view(torch.int32).clone(), out_sizes.clone(), out_comp.clone())
            if want is None:
                want = got
            else:
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (S, v)
                rows = got[1].tolist()
                assert all(torch.equal(got[2][i, :k], want[2][i, :k]) for i, k in enumerate(rows)), (S, v)
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
    print(f"scaled-reduce probe: {a.batch} x {a.words} bf16, P 10, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}; "
          f"per process the median of 3 runs, every variant in {a.runs} fresh processes of its own; us per step")
    print("  (a) reduce-compress   (b) reduce-compress, scale 1/3   (c) decode-reduce, mul_, cast-compress")
    for S in a.sources:
        per = {v: [r[str(S)] for r in runs[v]] for v in VARIANTS}
        mean = {v: statistics.mean(per[v]) for v in VARIANTS}
        spread = {v: (max(per[v]) - min(per[v])) / mean[v] for v in VARIANTS}
        cells = "   ".join(f"({v}) {mean[v]:7.1f} [{', '.join('%.1f' % x for x in per[v])}]" for v in VARIANTS)
        print(f"  S {S}: {cells}   b/a {mean['b'] / mean['a']:.3f}  b/c {mean['b'] / mean['c']:.3f}  "
              f"A/A spread (a) {100 * spread['a']:.1f} % (b) {100 * spread['b']:.1f} % (c) {100 * spread['c']:.1f} %")
    return 0


if __name__ == "__main__":
    sys.exit(main())
