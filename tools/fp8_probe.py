"""FP8 archives against their compositions and their bfloat16 siblings: 256 x 512 Ki float32 gradients N(0, 0.02^2),
factor 64, P 10, on cache-cold rotating buffer sets as bench.py's headline loop.  Every GROUP of paths runs in a fresh
process of its own (one child under its own time limit; the script stops at the first child that does not exit with 0),
its paths interleaved run by run inside that process so that a fused call and the composition it replaces see the same
machine:

  enc   (a) compress_data_cast(float8, scale=64)         (b) mul + .to(float8) + compress_data(False)
        (g) compress_data_cast(bfloat16)
  dec   (c) decompress_data_accumulate(float8, scale), stored    (d) decompress_data(False) + .float() + mul_
        (e) the same call, added                                 (f) ... + add_
        (h) decompress_data_accumulate(bfloat16 archive, scale), added
  plain (g), (h) and the raw-byte calls (i) compress_data(False) / (j) decompress_data(False) of the FP8 bytes: the paths
        this change must not move.  With --parent-lib naming a library built from the parent commit the group runs on
        both builds alternately, through ctypes (the op library links the tree's own core library).

    python tools/fp8_probe.py [--steps 40] [--warmup 8] [--sets 4] [--timeout 300] [--parent-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = {"enc": "abg", "dec": "cdefh", "plain": "ghij"}
LABEL = {"a": "compress_data_cast(float8, scale)", "b": "mul + .to(float8) + compress_data", "c": "decompress_data_accumulate(float8), stored",
         "d": "decompress_data + .float() + mul_", "e": "decompress_data_accumulate(float8), added", "f": "decompress_data + .float() + mul_ + add_",
         "g": "compress_data_cast(bfloat16)", "h": "decompress_data_accumulate(bfloat16), added", "i": "compress_data(False) of the FP8 bytes",
         "j": "decompress_data(False) of the FP8 bytes"}


def child(a):
    import torch

    sys.path.insert(0, ROOT)
    import dietgpu_amd as dg

    dg.prefer_torch_ops(a.route == "ops")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n, s = a.batch, a.words, 64.0
    dtype = torch.float8_e5m2 if a.fp8 == "e5m2" else torch.float8_e4m3fn
    gen = torch.Generator(device=dev).manual_seed(1234)
    sets, ratio = [], {}
    for k in range(a.sets):
        g = torch.randn((B, n), generator=gen, device=dev) * 0.02
        q = (g * s).to(dtype)
        st = {"g": g, "rows": [g[i] for i in range(B)], "q": q, "qrows": [q[i].view(torch.uint8) for i in range(B)],
              "acc": torch.zeros((B, n), device=dev), "f32": torch.empty((B, n), device=dev), "u8": torch.empty((B, n), dtype=torch.uint8, device=dev),
              "comp": torch.empty((B, dg.max_any_compressed_size(n)), dtype=torch.uint8, device=dev),
              "sizes": torch.empty((B,), dtype=torch.int32, device=dev)}
        st["accs"], st["u8rows"] = [st["acc"][i] for i in range(B)], [st["u8"][i] for i in range(B)]
        # the archives the decode paths read (by the composition, which every build has)
        comp, sizes, _ = dg.compress_data(False, st["qrows"])
        st["arch"] = [comp[i, : int(sizes[i])] for i in range(B)]
        bcomp, bsizes, _ = dg.compress_data_cast(st["rows"], torch.bfloat16)
        st["barch"], st["bcomp"], st["bsizes"] = [bcomp[i, : int(bsizes[i])] for i in range(B)], bcomp, bsizes
        if k == 0:
            ratio = {"fp8": float(sizes.sum()) / (n * B), "bf16": float(bsizes.sum()) / (n * B)}
        sets.append(st)

    def comp_fp8(st):
        torch.mul(st["g"], s, out=st["f32"])
        st["q"].copy_(st["f32"])  # (.to(float8) into a buffer that exists)
        dg.compress_data(False, st["qrows"], False, None, st["comp"], st["sizes"])

    def comp_dec(st, add):
        dg.decompress_data(False, st["arch"], st["u8rows"])
        torch.mul(st["u8"].view(dtype).float(), 1.0 / s, out=st["f32"])
        if add:
            st["acc"].add_(st["f32"])

    fns = {"a": lambda st: dg.compress_data_cast(st["rows"], dtype, None, st["comp"], st["sizes"], scale=s),
           "b": comp_fp8,
           "c": lambda st: dg.decompress_data_accumulate(st["arch"], st["accs"], False, dtype=dtype, scale=1.0 / s),
           "d": lambda st: comp_dec(st, False),
           "e": lambda st: dg.decompress_data_accumulate(st["arch"], st["accs"], True, dtype=dtype, scale=1.0 / s),
           "f": lambda st: comp_dec(st, True),
           "g": lambda st: dg.compress_data_cast(st["rows"], torch.bfloat16, None, st["bcomp"], st["bsizes"]),
           "h": lambda st: dg.decompress_data_accumulate(st["barch"], st["accs"], True, dtype=torch.bfloat16, scale=1.0 / s),
           "i": lambda st: dg.compress_data(False, st["qrows"], False, None, st["comp"], st["sizes"]),
           "j": lambda st: dg.decompress_data(False, st["arch"], st["u8rows"])}

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

    runs = {p: [] for p in GROUPS[a.group]}
    for _ in range(3):  # interleaved: every path once per round
        for p in GROUPS[a.group]:
            runs[p].append(timed(fns[p]))
    print("RESULT " + json.dumps({"runs": runs, "ratio": ratio}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--words", type=int, default=512 * 1024, help="float32 words per tensor")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--parent-lib", default=None, help="a core library built from the parent commit: the plain group runs on both builds")
    ap.add_argument("--group", choices=list(GROUPS), help="(child) the group to measure")
    ap.add_argument("--fp8", choices=["e4m3", "e5m2"], default="e4m3", help="(child)")
    ap.add_argument("--route", choices=["ops", "ctypes"], default="ops", help="(child)")
    a = ap.parse_args()
    if a.group:
        return child(a)
    print(f"fp8 probe: {a.batch} x {a.words} float32 N(0, 0.02^2), factor 64, P 10, {a.sets} rotating buffer sets, {a.steps} steps after "
          f"{a.warmup}, us per step, three interleaved runs per path, every group in a fresh process")
    jobs = [(g, t, "ops", None) for t in ("e4m3", "e5m2") for g in ("enc", "dec")]
    if a.parent_lib:
        jobs += [("plain", "e4m3", "ctypes", lib) for lib in (None, a.parent_lib, None, a.parent_lib)]
    for group, fp8, route, lib in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--group", group, "--fp8", fp8, "--route", route] + \
              [f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "sets", "batch", "words")]
        env = dict(os.environ, **({"DGPU_LIB": lib} if lib else {}))
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, env=env)
        except subprocess.TimeoutExpired:
            print(f"child {group} {fp8} ran into its time limit of {a.timeout} s; stopping")
            return 124
        if p.returncode != 0:
            print(f"child {group} {fp8} exited with {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            return p.returncode
        r = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])
        print(f"group {group}, {fp8}, route {route}, library {'parent commit' if lib else 'this tree'}:")
        for path, runs in r["runs"].items():
            print(f"  ({path}) {LABEL[path]:<44} {' / '.join('%.1f' % m for m in runs):>22}   median {sorted(runs)[1]:.1f}")
        print(f"  archive bytes per element: float8 {r['ratio']['fp8']:.3f}, bfloat16 {r['ratio']['bf16']:.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
