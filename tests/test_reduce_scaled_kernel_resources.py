"""Registers of k_ans_decode_reduce_mixed_scaled and k_ans_decode_reduce_mixed_stats_scaled, the forms of the mixed
decode-reduce kernels that multiply the last source's store by the call's scale (no GPU needed: hipcc cross-compiles).

The counting 16-bit form has no register to spare: 128 VGPRs with the scalar file full.  With the scale as a member of
its sink, or reloaded from the kernel arguments where it is used, a scalar is spilled into a VGPR lane (129: three waves
per SIMD); so that form reads the scale from LDS, one float per slot column behind the bins, through the address it
already holds.  The scaled forms are held to what tests/test_reduce_mixed_kernel_resources.py demands of the unscaled
ones, for the same instantiations: no scratch, no AGPRs, at most 128 VGPRs, four waves per SIMD -- and the LDS of the
counting form, 64 bytes larger, must still let two workgroups share a CU.  The scaled float32 form must not occupy less
than the unscaled one compiled beside it."""
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
template __global__ void k_ans_decode_reduce_mixed_scaled<10, kBFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_scaled<10, kBFloat16, kDecBlocksPerSmallTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_scaled<11, kFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_stats_scaled<10, kBFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_stats_scaled<10, kBFloat16, kDecBlocksPerSmallTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_stats_scaled<11, kFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_scaled<10, kFloat32, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed<10, kFloat32, kDecBlocksPerTile>(DecodeArgs);
static_assert(2u * decReduceStatsScaledLdsBytes(10, kBFloat16, kDecBlocksPerTile) <= 160u * 1024u, "two workgroups per CU");
static_assert(2u * decReduceStatsScaledLdsBytes(11, kFloat16, kDecBlocksPerTile) <= 160u * 1024u, "two workgroups per CU");
static_assert(decReduceStatsScaledLdsBytes(10, kBFloat16, kDecBlocksPerTile) == decReduceStatsLdsBytes(10, kBFloat16, kDecBlocksPerTile) + 64u, "one float per slot column");
static_assert(decReduceStatsScaledLdsBytes(10, kBFloat16, kDecBlocksPerSmallTile) == decReduceStatsLdsBytes(10, kBFloat16, kDecBlocksPerSmallTile) + 32u, "one float per slot column");
}
"""


def test_scaled_reduce_kernels_keep_four_waves_per_simd(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on PATH")
    src = tmp_path / "reduce_scaled_kernels.hip"
    src.write_text(SOURCE)
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "dietgpu_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "reduce_scaled_kernels.o"), str(src)], capture_output=True, text=True)
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
    fp32 = {k: v for k, v in kernels.items() if "k_ans_decode_reduce_mixed" in k and "ILi10ELj3E" in k}
    scaled = {k: v for k, v in kernels.items() if "_scaled" in k and k not in fp32}
    assert len(scaled) == 6, list(kernels)
    assert sum("k_ans_decode_reduce_mixed_stats_scaled" in k for k in scaled) == 3
    for name, r in scaled.items():
        print(name, r["VGPRs"], r["Occupancy [waves/SIMD]"])
        assert int(r["VGPRs"]) <= 128, f"{name}: {r['VGPRs']} VGPRs, fewer than four waves per SIMD"
        assert int(r["AGPRs"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 4, (name, r)
    assert len(fp32) == 2, list(kernels)
    (with_scale,) = [v for k, v in fp32.items() if "_scaled" in k]
    (without,) = [v for k, v in fp32.items() if "_scaled" not in k]
    print("float32", with_scale["VGPRs"], without["VGPRs"])
    assert int(with_scale["Occupancy [waves/SIMD]"]) >= int(without["Occupancy [waves/SIMD]"]), (with_scale, without)
    assert int(with_scale["AGPRs"]) == 0 and int(with_scale["ScratchSize [bytes/lane]"]) == 0, with_scale
