"""What the stochastic-rounding update of 16-bit parameters costs out of an archive: 256 x 512 Ki bf16 (and fp16)
archives, P 10, on cache-cold rotating buffer sets as bench.py's headline loop.

  (a) decompress_data_update(accumulate=True) with a device factor of 1/3 and a device seed: 2 bytes read and 2 written
      per word beside the archive;
  (b) decompress_data_accumulate(scale=, accumulate=True) into float32: 4 bytes read and 4 written per word;
  (c) the nearest composition: decompress_data_scaled into a 16-bit scratch, then add_ into the 16-bit parameters.  It
      rounds to nearest -- torch has no stochastic equivalent -- so it is a cost comparison, not an equivalent;
  (d) decompress_data: the plain decode, for the comparison with an earlier build.

First, in every process of leg (a): the first rows agree bit for bit with tests/sr_ref.py.  Buffer placement alone moves
these kernels by a few per cent between processes (docs/HISTORY.md section 3), so every variant is measured in a fresh
process of its own, `--runs` times: the runs of a variant are its A/A spread.  Every child process has its own time limit.

Besides the step time every process reports the KERNEL time of its leg's decode kernel (the library's per-kernel events,
as bench.py --full reads them, in a second pass of the same steps): the step time of a leg can be a host-submission
floor -- on the ctypes route a call marshals 512 pointers in Python, and the plain decode (d) then measures that and not
its kernel -- and the kernel time is what compares two libraries then.

--libs NAME ...: the legs are measured once per library, interleaved run by run ("base", or a file under
dietgpu_amd/lib/ made by tools/build_variant.py, selected with DGPU_LIB exactly as tools/ab.sh selects it -- that script
drives bench.py only, so the probe does the same interleaving itself; such legs take the ctypes route, so that every call
reaches the selected library: the op library is linked to the base one).  A library without the update call measures
(b) (c) (d).  The report begins with the command line that made it.

    python tools/decode_update_probe.py [--runs 2] [--steps 40] [--warmup 5] [--sets 4] [--limit 240] [--variants a b] [--libs base v_parent.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("a", "b", "c", "d")
DTYPES = ("bfloat16", "float16")
SCALE = 1.0 / 3.0
SEED = 0x0123456789ABCDEF
CHECK_ROWS = 4  # rows compared with the host reference


def child(a):
    import numpy as np
    import torch

    import dietgpu_amd as dg

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sr_ref as S

    if a.ctypes:
        dg.prefer_torch_ops(False)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n = a.batch, a.words
    res = {}
    for name in a.dtypes:
        dtype = getattr(torch, name)
        ft = S.BFLOAT16 if dtype == torch.bfloat16 else S.FLOAT16
        gen = torch.Generator(device=dev).manual_seed(4321)
        sets = []
        for _ in range(a.sets):
            x = torch.randn((B, n), generator=gen, device=dev).to(dtype)
            comp, sizes, _ = dg.compress_data(True, [x[i] for i in range(B)])
            rows = [comp[i, :k] for i, k in enumerate(sizes.tolist())]  # rows of one matrix: 16-byte aligned
            wide = a.variant == "b"
            par = torch.ones((B, n), dtype=torch.float32 if wide else dtype, device=dev)
            sets.append({"x": x[:CHECK_ROWS].clone() if not sets else None, "rows": rows, "par": par, "pars": [par[i] for i in range(B)]})
            del comp, x
        scratch = torch.empty((B, n), dtype=dtype, device=dev) if a.variant == "c" else None
        scratches = [scratch[i] for i in range(B)] if scratch is not None else None
        status = torch.zeros((B,), dtype=torch.uint8, device=dev)
        third = torch.tensor(SCALE, dtype=torch.float32, device=dev)
        seed = torch.tensor([SEED], dtype=torch.int64, device=dev)

        def run(st, v):
            if v == "a":
                dg.decompress_data_update(st["rows"], st["pars"], seed, third, True, 0, status, None)
            elif v == "b":
                dg.decompress_data_accumulate(st["rows"], st["pars"], True, None, status, None, dtype=dtype, scale=third)
            elif v == "c":
                dg.decompress_data_scaled(st["rows"], scratches, third, None, status, None)
                st["par"].add_(scratch)
            else:
                dg.decompress_data(True, st["rows"], st["pars"], False, None, status, None)

        if a.variant == "a":
            st = sets[0]
            src = st["x"].view(torch.int16).cpu().numpy().view(np.uint16)
            before = st["par"][:CHECK_ROWS].view(torch.int16).cpu().numpy().view(np.uint16)
            run(st, "a")
            assert bool(status.all())
            got = st["par"][:CHECK_ROWS].view(torch.int16).cpu().numpy().view(np.uint16)
            for i in range(CHECK_ROWS):
                assert np.array_equal(got[i], S.update_ref(src[i], ft, np.float32(SCALE), SEED, i, before[i])), f"{name}: (a) differs from the reference"

        def timed(v):
            for k in range(a.warmup):
                run(sets[k % a.sets], v)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(a.steps):
                run(sets[k % a.sets], v)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.steps * 1000.0  # us per step

        res[name] = statistics.median(timed(a.variant) for _ in range(3))
        # the decode kernel alone: per-kernel events on the launch stream, a second pass of the same steps
        L = dg.lib()
        L.dgpu_prof_reset()
        L.dgpu_prof_enable(1)
        for k in range(a.steps):
            run(sets[k % a.sets], a.variant)
        torch.cuda.synchronize()
        L.dgpu_prof_enable(0)
        buf = ctypes.create_string_buffer(1 << 16)
        prof = json.loads(buf.value.decode()) if L.dgpu_prof_summary(buf, len(buf)) > 0 else {}
        L.dgpu_prof_reset()
        res[name + " kernel"] = sum(r["total_ms"] / max(r["launches"], 1) for k, r in prof.items() if k.startswith("k_ans_decode")) * 1000.0
        del sets, scratch, scratches
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--words", type=int, default=512 * 1024)
    ap.add_argument("--dtypes", nargs="+", default=list(DTYPES), choices=DTYPES)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--variants", nargs="+", default=list(VARIANTS), choices=VARIANTS, help="the legs to measure")
    ap.add_argument("--libs", nargs="+", default=None, help="'base' or files under dietgpu_amd/lib/: every leg once per library, interleaved")
    ap.add_argument("--ctypes", action="store_true", help="take the ctypes route")
    ap.add_argument("--variant", choices=VARIANTS)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    args = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup), "--sets", str(a.sets),
            "--batch", str(a.batch), "--words", str(a.words), "--dtypes"] + list(a.dtypes)
    libs = a.libs or [None]
    if a.libs or a.ctypes:
        args.append("--ctypes")
    legs = [(v, lib) for v in VARIANTS if v in a.variants for lib in libs if not (v == "a" and lib not in (None, "base"))]
    runs = {leg: [] for leg in legs}
    for _ in range(a.runs):
        for leg in legs:  # a fresh process each: its own buffer placement, its own time limit
            v, lib = leg
            env = dict(os.environ)
            if lib not in (None, "base"):
                env["DGPU_LIB"] = os.path.join(ROOT, "dietgpu_amd", "lib", lib)
            try:
                p = subprocess.run(args + ["--variant", v], capture_output=True, text=True, timeout=a.limit, env=env)
            except subprocess.TimeoutExpired:
                sys.stderr.write(f"variant ({v}) did not finish within {a.limit} s\n")
                return 124
            if p.returncode != 0:  # nothing more is started after a child that failed
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                return p.returncode
            runs[leg].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
            sys.stderr.write(f"({v}) {lib or ''} {runs[leg][-1]}\n")
    print("python tools/decode_update_probe.py " + " ".join(sys.argv[1:]))
    print(f"decode-update probe: {a.batch} x {a.words} words, P 10, {a.sets} rotating buffer sets, {a.steps} steps after {a.warmup}; "
          f"per process the median of 3 runs, every variant in {a.runs} fresh processes of its own; us per step"
          + ("; ctypes route" if a.libs or a.ctypes else ""))
    print("  (a) decompress_data_update, accumulate, device factor 1/3, device seed   (b) decompress_data_accumulate(scale=), accumulate, "
          "float32   (c) decompress_data_scaled into a scratch, add_ (rounds to nearest)   (d) decompress_data")
    for name in a.dtypes:
        per = {leg: [r[name] for r in runs[leg]] for leg in legs}
        mean = {leg: statistics.mean(per[leg]) for leg in legs}
        tag = lambda leg: f"({leg[0]})" + (f" {leg[1]}" if leg[1] else "")
        print(f"  {name}: " + "   ".join(f"{tag(leg)} {mean[leg]:7.1f} [{', '.join('%.1f' % x for x in per[leg])}]" for leg in legs))
        print("    A/A spread " + " ".join(f"{tag(leg)} {100 * (max(per[leg]) - min(per[leg])) / mean[leg]:.1f} %" for leg in legs))
        kern = {leg: [r[name + " kernel"] for r in runs[leg]] for leg in legs}
        print("    decode kernel alone: " + "   ".join(f"{tag(leg)} {statistics.mean(kern[leg]):7.1f} [{', '.join('%.1f' % x for x in kern[leg])}]" for leg in legs))
        base = {leg[0]: mean[leg] for leg in legs if leg[1] in (None, "base")}
        if "a" in base and "b" in base:
            print(f"    a/b {base['a'] / base['b']:.3f}" + (f"  a/c {base['a'] / base['c']:.3f}" if "c" in base else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
