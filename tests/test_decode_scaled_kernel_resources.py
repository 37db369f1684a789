"""Registers of k_ans_decode_scaled, the form of the whole decode that multiplies every word by the member's factor before
it stores it (no GPU needed: hipcc cross-compiles).

The scaling happens in the sink, beside the row loop's dependent chain: it must cost no scratch, no AGPRs, and no
occupancy against k_ans_decode_accum of the same instantiation compiled beside it -- the form that today stores a decoded
tensor in another representation.  Its LDS is that of the whole decode.  The plain k_ans_decode instantiations are
compiled in the same file and must report what they reported before this form existed: adding a form to decodeTile
must not move the shipped decoder."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#            (P, float type, tile blocks)
INSTANCES = [(10, 2, 16), (10, 2, 4), (11, 1, 16), (10, 3, 16)]
# k_ans_decode on the commit before k_ans_decode_scaled was added: (VGPRs, waves per SIMD), from a build of that commit
PLAIN_BEFORE = {(10, 2, 16): (74, 6), (10, 2, 4): (74, 6), (11, 1, 16): (74, 6), (10, 3, 16): (64, 8)}
_FT = {1: "kFloat16", 2: "kBFloat16", 3: "kFloat32"}
SOURCE = """
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels_decode.h"
namespace dgpu {
""" + "".join(
    f"template __global__ void {k}<{p}, {_FT[ft]}, {tb}>(DecodeArgs);\n"
    for k in ("k_ans_decode_scaled", "k_ans_decode_accum", "k_ans_decode") for p, ft, tb in INSTANCES
) + """
// the form's LDS is that of the whole decode, nothing added
""" + "".join(
    f"static_assert(decScaledLdsBytes({p}, {_FT[ft]}, {tb}) == decLdsBytes({p}, {_FT[ft]}, {tb}), \"the LDS of the whole form\");\n"
    for p, ft, tb in INSTANCES
) + """}
"""


def _mangled(kernel, p, ft, tb):
    return f"{len(kernel)}{kernel}ILi{p}ELj{ft}ELj{tb}EE"


def test_scaled_decoder_costs_no_occupancy_and_leaves_the_plain_decoder_alone(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on PATH")
    src = tmp_path / "decode_scaled_kernels.hip"
    src.write_text(SOURCE)
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "dietgpu_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "decode_scaled_kernels.o"), str(src)], capture_output=True, text=True)
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

    def of(kernel, inst):
        (r,) = [v for k, v in kernels.items() if _mangled(kernel, *inst) in k]
        return r

    for inst in INSTANCES:
        scaled, accum, plain = of("k_ans_decode_scaled", inst), of("k_ans_decode_accum", inst), of("k_ans_decode", inst)
        waves = lambda r: int(r["Occupancy [waves/SIMD]"])
        print(inst, "scaled", scaled["VGPRs"], waves(scaled), "accum", accum["VGPRs"], waves(accum), "plain", plain["VGPRs"], waves(plain))
        assert int(scaled["AGPRs"]) == 0 and int(scaled["ScratchSize [bytes/lane]"]) == 0, (inst, scaled)
        assert waves(scaled) >= waves(accum), (inst, scaled, accum)
        assert (int(plain["VGPRs"]), waves(plain)) == PLAIN_BEFORE[inst], (inst, plain)
        assert int(plain["AGPRs"]) == 0 and int(plain["ScratchSize [bytes/lane]"]) == 0, (inst, plain)


def test_the_launch_uses_the_lds_the_static_assert_speaks_of():
    text = open(os.path.join(ROOT, "dietgpu_amd", "csrc", "kernel_variants.h")).read()
    # (the row of the decode forms' table, and what every row of it becomes)
    assert "X(kWholeScaled, k_ans_decode_scaled, floatsOnly, decScaledLdsBytes(P, T, TB))" in text
    assert "return {kernel<P, T, TB>, decThreads(TB), ldsBytes, #kernel};" in text
