"""Registers of k_ans_decode_reduce_mixed and k_ans_decode_reduce_mixed_stats, the forms of the decode-reduce kernels
whose sources are archives or raw rows (no GPU needed: hipcc cross-compiles).

A raw source takes its turn in the source loop before anything of the archive path is set up, and the kind of a source
travels in its address: beside decodeBlock in one block, the raw path's values stretched the live ranges across the row
loop (167 VGPRs), and a separate array of kinds cost the counting bf16 form the one scalar register it had left (a
VGPR lane took it: 129).  The mixed forms are held to what tests/test_reduce_kernel_resources.py and
tests/test_reduce_compress_kernel_resources.py demand of the plain ones, for the same instantiations: no scratch, no
AGPRs, at most 128 VGPRs, four waves per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = """
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels_decode.h"
namespace dgpu {
template __global__ void k_ans_decode_reduce_mixed<10, kBFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed<10, kBFloat16, kDecBlocksPerSmallTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed<11, kFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_stats<10, kBFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_stats<10, kBFloat16, kDecBlocksPerSmallTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_stats<11, kFloat16, kDecBlocksPerTile>(DecodeArgs);
static_assert(2u * decReduceStatsLdsBytes(10, kBFloat16, kDecBlocksPerTile) <= 160u * 1024u, "two workgroups per CU");
static_assert(2u * decReduceStatsLdsBytes(11, kFloat16, kDecBlocksPerTile) <= 160u * 1024u, "two workgroups per CU");
}
"""


def test_sixteen_bit_mixed_reduce_kernels_keep_four_waves_per_simd(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on PATH")
    src = tmp_path / "reduce_mixed_kernels.hip"
    src.write_text(SOURCE)
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "dietgpu_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "reduce_mixed_kernels.o"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    kernels, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass", line)
        if not m:
            continue
        key, _, value = m.group(1).strip().partition(":")
        if key == "Function Name":
            cur = kernels.setdefault(value.strip(), {})
        elif cur is not None:
            cur[key.strip()] = value.strip()
    mixed = {k: v for k, v in kernels.items() if "k_ans_decode_reduce_mixed" in k}
    assert len(mixed) == 6, list(kernels)
    assert sum("k_ans_decode_reduce_mixed_stats" in k for k in mixed) == 3
    for name, r in mixed.items():
        print(name, r["VGPRs"], r["Occupancy [waves/SIMD]"])
        assert int(r["VGPRs"]) <= 128, f"{name}: {r['VGPRs']} VGPRs, fewer than four waves per SIMD"
        assert int(r["AGPRs"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 4, (name, r)
