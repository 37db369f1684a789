"""Registers of k_ans_decode_reduce (no GPU needed: hipcc cross-compiles).

decodeReduceTile derives everything a lane computes from its index INSIDE the source loop, behind an empty asm the
compiler cannot see through.  Hoisted out of the loop those values stayed in registers across decodeBlock: 151 VGPRs,
three waves per SIMD -- one 512-thread workgroup per CU where k_ans_decode_accum has two.  A SIMD has 512 VGPRs per
lane, so four waves need at most 128 each; that, and no scratch, is asserted for the 16-bit forms of both tile sizes
(the float32 forms have no store buffer groups in registers and sit far below).  The two kernels are instantiated in a
translation unit of their own: seconds, not the minutes of the whole library."""
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
template __global__ void k_ans_decode_reduce<10, kBFloat16, kDecBlocksPerTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce<10, kBFloat16, kDecBlocksPerSmallTile>(DecodeArgs);
template __global__ void k_ans_decode_reduce<11, kFloat16, kDecBlocksPerTile>(DecodeArgs);
}
"""


def test_sixteen_bit_reduce_kernels_keep_four_waves_per_simd(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on PATH")
    src = tmp_path / "reduce_kernels.hip"
    src.write_text(SOURCE)
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "dietgpu_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "reduce_kernels.o"), str(src)], capture_output=True, text=True)
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
    reduce = {k: v for k, v in kernels.items() if "k_ans_decode_reduce" in k}
    assert len(reduce) == 3, list(kernels)
    for name, r in reduce.items():
        print(name, r["VGPRs"], r["Occupancy [waves/SIMD]"])
        assert int(r["VGPRs"]) <= 128, f"{name}: {r['VGPRs']} VGPRs, fewer than four waves per SIMD"
        assert int(r["AGPRs"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 4, (name, r)
