#!/usr/bin/env python3
"""A fixed list of compress + decompress calls that reaches every branch of the kernel selection
(csrc/kernel_variants.h), and the digest of the launches a profiler saw them make.  Two builds of the library select
the same kernels when their digests agree:

    rocprofv3 --kernel-trace -d DIR -o seq -- python tools/launch_sequence.py          (once per build)
    python tools/launch_sequence.py --digest DIR/seq_results.db [--lines OUT.txt]

The calls: raw bytes, fp16, bf16 and fp32; probBits 9, 10 and 11; elements of one block (the pair kernels) and tiles
of 2, 4 and 8 blocks, the 8-block ones with at most 32 tiles per element (wide stage) and with more; the encoder's
dispatch left to the policy, forced persistent and forced to the hardware; ordinary histogram loads; one batch of size
classes (1 large + many small) and one ragged batch; a caller-supplied histogram.  The digest is over the lines
(kernel name with its template arguments, grid, workgroup size, LDS bytes) in launch order."""
import argparse
import ctypes as C
import hashlib
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (words per element, elements): one block; tiles of 2 / 4 blocks, more of them than fit on the chip at once; 8-block
# tiles with 4 tiles per element; with 40 tiles per element, more tiles than resident workgroups
SHAPES = [(3000, 64), (8000, 2048), (16000, 2048), (100000, 16), (40 * 32768, 64)]


def digest(db, lines_out):
    con = sqlite3.connect(db)
    cols = [d[1] for d in con.execute("pragma table_info(kernels)")]
    want = [c for c in ("name", "grid_x", "grid_y", "workgroup_x", "lds_size") if c in cols]
    rows = con.execute(f"select {', '.join(want)} from kernels where name like '%dgpu::%' order by start").fetchall()
    lines = [" ".join(str(x) for x in r) for r in rows]
    if lines_out:
        with open(lines_out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} launches, {len(set(lines))} distinct, sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}")


def main():
    import torch

    import dietgpu_amd as dg

    L = dg.lib()
    dg.ops.prefer_torch_ops(False)  # (prob_bits and the debug setters act on the core library: one route for all)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)

    def tensors(dtype, sizes):
        if dtype == torch.uint8:
            return [(torch.randn([n], generator=g, device=dev) * 12).to(torch.int8).view(torch.uint8) for n in sizes]
        return [torch.randn([n], generator=g, device=dev).to(dtype) for n in sizes]

    def round_trip(ts, prob_bits):
        is_float = ts[0].dtype != torch.uint8
        comp, sizes, _ = dg.compress_data(is_float, ts, False, prob_bits=prob_bits)
        outs = [torch.empty_like(t) for t in ts]
        dg.decompress_data(is_float, [comp[i, : int(s)] for i, s in enumerate(sizes.tolist())], outs, False, prob_bits=prob_bits)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(ts, outs)), "round trip mismatch"

    dtypes = (torch.uint8, torch.float16, torch.bfloat16, torch.float32)
    for dtype in dtypes:
        for words, batch in SHAPES:
            ts = list(tensors(dtype, [words * batch])[0].view(batch, words).unbind(0))
            for prob_bits in (9, 10, 11):
                for dispatch in (-1, 0, 1):
                    L.dgpu_debug_set_encoder_dispatch(dispatch)
                    round_trip(ts, prob_bits)
            L.dgpu_debug_set_encoder_dispatch(-1)
            L.dgpu_set_histogram_load_policy(1)
            round_trip(ts, 10)
            L.dgpu_set_histogram_load_policy(-1)
    for dtype in (torch.uint8, torch.bfloat16):
        round_trip(tensors(dtype, [2 * 1024 * 1024] + [1000 + 37 * i for i in range(200)]), 10)  # size classes
        round_trip(tensors(dtype, [64 * 1024 + 15000 * i for i in range(64)]), 10)  # ragged

    # caller-supplied histogram (stand-alone normalisation)
    n, b = 50000, 4
    x = tensors(torch.uint8, [n * b])[0]
    hist = torch.zeros([b, 256], dtype=torch.int32, device=dev)
    stride = int(L.dgpu_ans_max_compressed_size(n))
    arch = torch.zeros([b, stride], dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.dgpu_ans_histogram_batch_stride(b, p(x), n, n, p(hist), st) == 0
    assert L.dgpu_ans_encode_batch_stride(None, 0, None, 10, 0, b, p(x), n, n, p(hist), p(arch), stride, None, st) == 0
    out = torch.empty_like(x)
    assert L.dgpu_ans_decode_batch_stride(None, 0, None, 10, 0, b, p(arch), stride, p(out), n, n, None, None, st, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, x), "round trip mismatch (caller-supplied histogram)"
    print("launch sequence done")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--digest", default=None, help="the profiler's results database of a run of this script")
    ap.add_argument("--lines", default=None, help="with --digest: write the launch lines here")
    a = ap.parse_args()
    if a.digest:
        digest(a.digest, a.lines)
    else:
        main()
