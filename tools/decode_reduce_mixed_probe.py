"""What a raw source costs: 32 x 512 Ki bf16 accumulators, S sources each, P 10, summed into float32 on cache-cold
rotating buffer sets as bench.py's headline loop.  For S in 2, 4, 8, alternating within one process:

  (a)  decompress_data_reduce, every source an archive;
  (b0) decompress_data_reduce_mixed, source 0 a raw bf16 row (stored: the first source of the sum);
  (bL) decompress_data_reduce_mixed, source S - 1 a raw row (added last);

and the same three for decompress_data_reduce_compress / decompress_data_reduce_compress_mixed.  All leave the same bits
(asserted first).  Buffer placement alone moves these kernels by a few per cent between processes (docs/HISTORY.md
section 3), so the measurement is repeated in fresh processes (--processes) and the report gives every process's
figures, their median, and the spread of (a) between processes -- the margin against which (b) is read.  Prints one
text report (the figures of DESIGN.md section 5, profiles/decode_reduce_mixed_32x512Ki.txt).

    python tools/decode_reduce_mixed_probe.py [--processes 3] [--steps 40] [--warmup 5] [--sets 4]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ("a", "b0", "bL")


def child(a):
    import torch

    import dietgpu_amd as dg

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n, smax = a.batch, a.words, max(a.sources)
    gen = torch.Generator(device="cpu").manual_seed(4321)
    sets = []
    for _ in range(a.sets):
        archs, raws = [], []  # [source][member]
        for _s in range(smax):
            x = torch.randn((B, n), generator=gen).to(torch.bfloat16).to(dev)
            comp, sizes, _ = dg.compress_data(True, [x[i] for i in range(B)])
            archs.append([comp[i, :k] for i, k in enumerate(sizes.tolist())])  # rows of one matrix: 16-byte aligned
            raws.append([x[i] for i in range(B)])
        acc = torch.zeros((B, n), dtype=torch.float32, device=dev)
        st = {"acc": acc, "acc_rows": [acc[i] for i in range(B)], "ins": {}}
        for S in a.sources:
            for v, raw_at in (("a", None), ("b0", 0), ("bL", S - 1)):
                st["ins"][S, v] = [[raws[s][i] if s == raw_at else archs[s][i] for s in range(S)] for i in range(B)]
        sets.append(st)
    status = torch.zeros((B,), dtype=torch.uint8, device=dev)
    cols = dg.max_float_compressed_size(torch.empty(0, dtype=torch.bfloat16), n)
    out_comp = torch.empty((B, cols), dtype=torch.uint8, device=dev)
    out_sizes = torch.empty((B,), dtype=torch.int32, device=dev)

    def reduce(st, S, v):
        f = dg.decompress_data_reduce if v == "a" else dg.decompress_data_reduce_mixed
        f(st["ins"][S, v], st["acc_rows"], False, None, status, None, dtype=torch.bfloat16)

    def reduce_compress(st, S, v):
        f = dg.decompress_data_reduce_compress if v == "a" else dg.decompress_data_reduce_compress_mixed
        f(st["ins"][S, v], st["acc_rows"], False, None, status, None, out_comp, out_sizes, dtype=torch.bfloat16)

    def timed(fn, S, v):
        for k in range(a.warmup):
            fn(sets[k % a.sets], S, v)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.steps):
            fn(sets[k % a.sets], S, v)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps * 1000.0  # us per step

    # bit-exact first
    for S in a.sources:
        for st in sets:
            for fn in (reduce, reduce_compress):
                want = None
                for v in VARIANTS:
                    st["acc"].fill_(float("nan"))
                    fn(st, S, v)
                    assert bool(status.all()), (S, v)
                    got = (st["acc"].view(torch.int32).clone(), out_sizes.clone(), out_comp.clone() if fn is reduce_compress else None)
                    if want is None:
                        want = got
                    else:
                        assert torch.equal(got[0], want[0]), (S, v)
                        if fn is reduce_compress:
                            assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), (S, v)
    res = {}
    for name, fn in (("reduce", reduce), ("reduce_compress", reduce_compress)):
        for S in a.sources:
            rows = [[timed(fn, S, v) for v in VARIANTS] for _ in range(3)]  # alternating
            res[f"{name} {S}"] = [sorted(r[i] for r in rows)[1] for i in range(len(VARIANTS))]
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--words", type=int, default=512 * 1024)
    ap.add_argument("--sources", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    args = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup), "--sets", str(a.sets),
            "--batch", str(a.batch), "--words", str(a.words), "--sources"] + [str(s) for s in a.sources]
    for _ in range(a.processes):  # a fresh process each: its own buffer placement
        p = subprocess.run(args, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            return p.returncode
        runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    print(f"decode-reduce-mixed probe: {a.batch} x {a.words} bf16, P 10, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}; "
          f"per process the median of 3 alternating runs, {a.processes} fresh processes; us per step")
    print("  (a) all sources archives (the plain call)   (b0) source 0 raw   (bL) source S-1 raw")
    for key in runs[0]:
        per = [[r[key][i] for r in runs] for i in range(len(VARIANTS))]
        med = [statistics.median(p) for p in per]
        spread = (max(per[0]) - min(per[0])) / med[0]
        cells = "   ".join(f"({v}) {med[i]:7.1f} [{', '.join('%.1f' % x for x in per[i])}]" for i, v in enumerate(VARIANTS))
        print(f"  {key:>18}: {cells}   b0/a {med[1] / med[0]:.3f}  bL/a {med[2] / med[0]:.3f}  spread of (a) {100 * spread:.1f} %")
    return 0


if __name__ == "__main__":
    sys.exit(main())
