"""Registers of k_ans_decode_reduce_mixed_norm and k_ans_decode_reduce_mixed_stats_norm, the forms of the scaled mixed
decode-reduce kernels that also measure the words they leave (no GPU needed: hipcc cross-compiles).

The counting 16-bit form has no register to spare: 128 VGPRs with the scalar file full.  Measuring where the words are
stored (a float64 partial in a per-lane LDS slot beside each store) costs it 3 to 5 VGPRs and a dozen spilled scalars; so
the norm forms measure a tile when its last source is in the accumulator, in a pass that reads everything it needs from a
ReduceNormTile in LDS and keeps nothing alive across the source loop.  They are held to what
tests/test_reduce_scaled_kernel_resources.py demands of the scaled forms, for the same instantiations: no scratch, no
AGPRs, no spilled scalar, at most 128 VGPRs, four waves per SIMD -- and the LDS of the counting form, a ReduceNormTile
larger, must still let two workgroups share a CU.  The float32 norm form must not occupy less than the scaled one
compiled beside it."""
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
template __global__ void k_ans_decode_reduce_mixed_norm<10, kBFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_norm<10, kBFloat16, kDecBlocksPerSmallTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_norm<11, kFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_stats_norm<10, kBFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_stats_norm<10, kBFloat16, kDecBlocksPerSmallTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_stats_norm<11, kFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_norm<10, kFloat32, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce_mixed_scaled<10, kFloat32, kDecBlocksPerTile>(DecodeArgs);
static_assert(2u * decReduceNormLdsBytes(10, kBFloat16, kDecBlocksPerTile, true) <= 160u * 1024u, "two workgroups per CU");
static_assert(2u * decReduceNormLdsBytes(11, kFloat16, kDecBlocksPerTile, true) <= 160u * 1024u, "two workgroups per CU");
static_assert(decReduceNormLdsBytes(10, kBFloat16, kDecBlocksPerTile, true) == decReduceStatsScaledLdsBytes(10, kBFloat16, kDecBlocksPerTile) + sizeof(ReduceNormTile), "");
static_assert(decReduceNormLdsBytes(10, kBFloat16, kDecBlocksPerSmallTile, false) == decLdsBytes(10, kBFloat16, kDecBlocksPerSmallTile) + sizeof(ReduceNormTile), "");
static_assert(sizeof(ReduceNormTile) == 32u, "");
}
"""


def test_norm_reduce_kernels_keep_four_waves_per_simd(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on PATH")
    src = tmp_path / "reduce_norm_kernels.hip"
    src.write_text(SOURCE)
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "dietgpu_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "reduce_norm_kernels.o"), str(src)], capture_output=True, text=True)
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
    norm = {k: v for k, v in kernels.items() if "k_ans_decode_reduce_mixed" in k and "_norm" in k and k not in fp32}
    assert len(norm) == 6, list(kernels)
    assert sum("k_ans_decode_reduce_mixed_stats_norm" in k for k in norm) == 3
    for name, r in norm.items():
        print(name, r["VGPRs"], r["Occupancy [waves/SIMD]"])
        assert int(r["VGPRs"]) <= 128, f"{name}: {r['VGPRs']} VGPRs, fewer than four waves per SIMD"
        assert int(r["AGPRs"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r.get("SGPRs Spill", r.get("SGPR Spill", "0"))) == 0, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 4, (name, r)
    assert len(fp32) == 2, list(kernels)
    (with_norm,) = [v for k, v in fp32.items() if "_norm" in k]
    (scaled,) = [v for k, v in fp32.items() if "_scaled" in k]
    print("float32", with_norm["VGPRs"], scaled["VGPRs"])
    assert int(with_norm["Occupancy [waves/SIMD]"]) >= int(scaled["Occupancy [waves/SIMD]"]), (with_norm, scaled)
    assert int(with_norm["AGPRs"]) == 0 and int(with_norm["ScratchSize [bytes/lane]"]) == 0, with_norm
