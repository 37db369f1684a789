"""Registers of k_ans_decode_reduce_stats, the counting form of the decode-reduce kernel (no GPU needed: hipcc
cross-compiles).

The counting form carries, beside everything k_ans_decode_reduce holds across decodeBlock, the LDS address of the lane's
bin column, and on the last source rounds and counts eight sums per lane and group.  It is held to what the plain kernel
is held to in tests/test_reduce_kernel_resources.py: no scratch, no AGPRs, at most 128 VGPRs -- four waves per SIMD, two
512-thread workgroups per CU (the bins bring the 16-block form to 64 KiB of LDS, two of which fit the CU's 160 KiB).
The three kernels are instantiated in a translation unit of their own: seconds, not the minutes of the whole library."""
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
template __global__ void k_ans_decode_reduce_stats<10, kBFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_stats<10, kBFloat16, kDecBlocksPerSmallTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_stats<11, kFloat16, kDecBlocksPerTile>(DecodeArgs);
static_assert(2u * decReduceStatsLdsBytes(10, kBFloat16, kDecBlocksPerTile) <= 160u * 1024u, "two workgroups per CU");
static_assert(2u * decReduceStatsLdsBytes(11, kFloat16, kDecBlocksPerTile) <= 160u * 1024u, "two workgroups per CU");
}
"""


def test_sixteen_bit_counting_reduce_kernels_keep_four_waves_per_simd(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on PATH")
    src = tmp_path / "reduce_stats_kernels.hip"
    src.write_text(SOURCE)
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "dietgpu_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "reduce_stats_kernels.o"), str(src)], capture_output=True, text=True)
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
    stats = {k: v for k, v in kernels.items() if "k_ans_decode_reduce_stats" in k}
    assert len(stats) == 3, list(kernels)
    for name, r in stats.items():
        print(name, r["VGPRs"], r["Occupancy [waves/SIMD]"])
        assert int(r["VGPRs"]) <= 128, f"{name}: {r['VGPRs']} VGPRs, fewer than four waves per SIMD"
        assert int(r["AGPRs"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 4, (name, r)
