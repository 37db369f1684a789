"""XOR-delta archives against their compositions: 256 x 1 MiB of bytes -- bf16 N(0, 0.02) words, a quarter of them moved
by one ulp against the base -- P 10, on cache-cold rotating buffer sets as bench.py's headline loop.  Six paths, each
measured in a FRESH process of its own (one child under its own time limit; the script stops at the first child that does
not exit with 0), interleaved in one command:

  (a) compress_data_delta;
  (b) torch.bitwise_xor into a scratch + compress_data(False, ...): what a user has without the call;
  (c) decompress_data_delta in place;
  (d) decompress_data(False, ...) into a scratch + bitwise_xor_ into the base;
  (e) compress_data(False, ...) of the XOR-ed bytes alone;   (f) decompress_data(False, ...) alone.

Every child also reports the library's kernels alone (dgpu_prof_summary) and the archive sizes: the delta archive and the
float archive (compress_data(True, ...)) of the same tensors against the tensors' bytes.

    python tools/delta_probe.py [--steps 60] [--warmup 10] [--sets 4] [--timeout 240] [--paths a,b,c,d,e,f] [--route ops|ctypes]

--paths b,d,e,f --route ctypes with DGPU_LIB naming a library built from an earlier revision measures that build on the
same route (the op library links the tree's own core library, so an A/B goes through ctypes on both sides).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = {"a": "compress_data_delta", "b": "bitwise_xor + compress_data", "c": "decompress_data_delta, in place",
         "d": "decompress_data + bitwise_xor_", "e": "compress_data alone", "f": "decompress_data alone"}


def child(a):
    import torch

    sys.path.insert(0, ROOT)
    import dietgpu_amd as dg

    dg.prefer_torch_ops(a.route == "ops")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n = a.batch, a.bytes // 2  # words per tensor
    gen = torch.Generator(device=dev).manual_seed(1234)
    cap = dg.max_any_compressed_size(2 * n)
    temp = torch.empty((max(int(dg.lib().dgpu_ans_encode_temp_bytes(B, 2 * n)), int(dg.lib().dgpu_ans_decode_temp_bytes(B, 2 * n, 10))),),
                       dtype=torch.uint8, device=dev)
    sets, ratio = [], {}
    for k in range(a.sets):
        base = (torch.randn((B, n), generator=gen, device=dev) * 0.02).to(torch.bfloat16).view(torch.int16)
        new = base + (torch.randint(0, 4, (B, n), generator=gen, device=dev) == 0).to(torch.int16)
        s = {"new": [new[i] for i in range(B)], "base": [base[i] for i in range(B)], "basem": base, "newm": new,
             "x": torch.bitwise_xor(new, base), "comp": torch.empty((B, cap), dtype=torch.uint8, device=dev),
             "sizes": torch.empty((B,), dtype=torch.int32, device=dev), "scratch": torch.empty_like(new)}
        s["xrows"], s["srows"] = [s["x"][i] for i in range(B)], [s["scratch"][i] for i in range(B)]
        # the archives the decode paths read (by the composition, which every build has)
        dg.compress_data(False, s["xrows"], False, temp, s["comp"], s["sizes"])
        sizes = s["sizes"].tolist()
        s["rows"] = [s["comp"][i, : sizes[i]] for i in range(B)]
        if k == 0:
            _, fsizes, _ = dg.compress_data(True, [r.view(torch.bfloat16) for r in s["new"]])
            ratio = {"delta": sum(sizes) / (2.0 * n * B), "float": float(fsizes.sum()) / (2.0 * n * B)}
        sets.append(s)

    def delta_enc(s):
        dg.compress_data_delta(s["new"], s["base"], s["comp"], s["sizes"])

    def xor_enc(s):
        torch.bitwise_xor(s["newm"], s["basem"], out=s["scratch"])
        dg.compress_data(False, s["srows"], False, temp, s["comp"], s["sizes"])

    def delta_dec(s):  # (in place: the base flips between the two tensors step after step, the work does not change)
        dg.decompress_data_delta(s["rows"], s["base"])

    def xor_dec(s):
        dg.decompress_data(False, s["rows"], s["srows"], False, temp)
        s["basem"].bitwise_xor_(s["scratch"])

    def plain_enc(s):
        dg.compress_data(False, s["xrows"], False, temp, s["comp"], s["sizes"])

    def plain_dec(s):
        dg.decompress_data(False, s["rows"], s["srows"], False, temp)

    fn = {"a": delta_enc, "b": xor_enc, "c": delta_dec, "d": xor_dec, "e": plain_enc, "f": plain_dec}[a.path]

    def timed():
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

    runs = [timed() for _ in range(3)]
    L = dg.lib()
    L.dgpu_prof_reset()
    L.dgpu_prof_enable(1)
    for k in range(a.steps):
        fn(sets[k % a.sets])
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    L.dgpu_prof_summary(buf, len(buf))
    L.dgpu_prof_enable(0)
    prof = json.loads(buf.value.decode())
    kern = {k: v["total_ms"] / v["launches"] * 1000.0 for k, v in prof.items() if v.get("launches")}
    print("RESULT " + json.dumps({"path": a.path, "runs": runs, "ratio": ratio, "kernels": kern}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bytes", type=int, default=1 << 20, help="bytes per tensor")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--paths", default="a,b,c,d,e,f", help="the paths to measure, e.g. b,d")
    ap.add_argument("--route", choices=["ops", "ctypes"], default="ops", help="torch ops (the default route) or ctypes")
    ap.add_argument("--path", choices=list(LABEL), help="(child) the path to measure")
    a = ap.parse_args()
    if a.path:
        return child(a)
    paths = [p for p in a.paths.split(",") if p]
    lib = os.environ.get("DGPU_LIB")
    print(f"delta probe: {a.batch} x {a.bytes} bytes (bf16, a quarter of the words moved one ulp), P 10, {a.sets} rotating buffer sets, "
          f"{a.steps} steps after {a.warmup}, median of 3 runs, every path in a fresh process, route {a.route}"
          + (f", library {os.path.basename(os.path.dirname(lib))}/{os.path.basename(lib)}" if lib else ""))
    res = {}
    for path in paths + paths[-2::-1]:  # there and back: every path but the last twice, the spread between two processes shows
        cmd = [sys.executable, os.path.abspath(__file__), "--path", path] + [f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "sets", "batch", "bytes", "route")]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"child {path} ran into its time limit of {a.timeout} s; stopping")
            return 124
        if p.returncode != 0:
            print(f"child {path} exited with {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            return p.returncode
        line = next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))
        res.setdefault(path, []).append(json.loads(line[7:]))
    med = {k: [sorted(r["runs"])[1] for r in v] for k, v in res.items()}
    for path in paths:
        print(f"  ({path}) {LABEL[path]:<34} {' / '.join('%.1f' % m for m in med[path]):>16} us per step")
    for x, y in (("a", "b"), ("c", "d"), ("a", "e"), ("c", "f")):
        if x in med and y in med:
            print(f"  ({x}) / ({y}) = {min(med[x]) / min(med[y]):.3f}   ({x}) - ({y}) = {min(med[x]) - min(med[y]):.1f} us")
    r = res[paths[0]][0]["ratio"]
    print(f"  archive / tensor bytes: delta {r['delta']:.3f}, plain float archive {r['float']:.3f}")
    for path in paths:
        k = res[path][0]["kernels"]
        print(f"  library kernels alone, path ({path}): " + ", ".join(f"{n} {t:.1f} us" for n, t in sorted(k.items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
