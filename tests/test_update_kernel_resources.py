"""Registers of k_ans_decode_update, the decode that multiplies every word by the member's factor, adds the 16-bit tensor
word and rounds stochastically (no GPU needed: hipcc cross-compiles).

The multiply, the add, the four mixes per lane and group and the rounding sit in the sink, beside the row loop's dependent
chain: they must cost no scratch, no AGPRs, and no occupancy against k_ans_decode_accum_scaled of the same instantiation
compiled beside it -- the new sink carries 8 tensor words per group in 4 registers where that one carries 8 accumulator
words in 8, so it must need fewer VGPRs (the check of "half that kernel's accumulator registers").  The multiply and the
add must stay two instructions; the 16-byte stores are as many as k_ans_decode_scaled's, and 16-byte loads are added for
the tensor words.  k_ans_decode,
k_ans_decode_scaled and k_ans_decode_accum_scaled are compiled in the same file and must report what they reported before
this form existed: the new form is a sink of its own and a compile-time flag of decodeTile."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#            (P, float type, tile blocks)
INSTANCES = [(10, 2, 16), (10, 2, 4), (11, 1, 16)]
# (VGPRs, waves per SIMD) on the commit before k_ans_decode_update was added, from a build of that commit
BEFORE = {
    "k_ans_decode": {(10, 2, 16): (74, 6), (10, 2, 4): (74, 6), (11, 1, 16): (74, 6)},
    "k_ans_decode_scaled": {(10, 2, 16): (76, 6), (10, 2, 4): (75, 6), (11, 1, 16): (76, 6)},
    "k_ans_decode_accum_scaled": {(10, 2, 16): (103, 4), (10, 2, 4): (110, 4), (11, 1, 16): (104, 4)},
}
NEW = "k_ans_decode_update"
_FT = {1: "kFloat16", 2: "kBFloat16"}
SOURCE = """
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels_decode.h"
namespace dgpu {
""" + "".join(
    f"template __global__ void {k}<{p}, {_FT[ft]}, {tb}>(DecodeArgs);\n"
    for k in (NEW,) + tuple(BEFORE) for p, ft, tb in INSTANCES
) + """}
"""


def _mangled(kernel, p, ft, tb):
    return f"{len(kernel)}{kernel}ILi{p}ELj{ft}ELj{tb}EE"


def test_update_costs_no_occupancy_stays_unfused_and_leaves_the_others_alone(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on PATH")
    src = tmp_path / "update_kernels.hip"
    asm = tmp_path / "update_kernels.s"
    src.write_text(SOURCE)
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "dietgpu_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(asm), str(src)], capture_output=True, text=True)
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

    waves = lambda r: int(r["Occupancy [waves/SIMD]"])
    for inst in INSTANCES:
        new, accum = of(NEW, inst), of("k_ans_decode_accum_scaled", inst)
        print(inst, NEW, new["VGPRs"], waves(new), *[f"{k} {of(k, inst)['VGPRs']} {waves(of(k, inst))}" for k in BEFORE])
        assert int(new["AGPRs"]) == 0 and int(new["ScratchSize [bytes/lane]"]) == 0, (inst, new)
        assert waves(new) >= waves(accum), (inst, new, accum)
        assert int(new["VGPRs"]) < int(accum["VGPRs"]), (inst, new, accum)
        for kernel, before in BEFORE.items():
            r = of(kernel, inst)
            assert (int(r["VGPRs"]), waves(r)) == before[inst], (kernel, inst, r)
            assert int(r["AGPRs"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (kernel, inst, r)

    # the bodies of the new kernels: a float32 multiply and a float32 add, and nothing that fuses the two
    parts = re.split(r"^(_ZN4dgpu\w+):[^\n]*\n", asm.read_text(), flags=re.M)
    bodies = {parts[i]: parts[i + 1].split(".Lfunc_end")[0] for i in range(1, len(parts), 2)}
    for inst in INSTANCES:
        (body,) = [b for k, b in bodies.items() if _mangled(NEW, *inst) in k]
        fused = re.findall(r"^\s+(v_(?:pk_)?(?:fma|fmac|mad|mac)\w*_f32\w*)", body, flags=re.M)
        assert not fused, (inst, sorted(set(fused)))
        assert re.search(r"^\s+v_(?:pk_)?mul_f32", body, flags=re.M), inst
        assert re.search(r"^\s+v_(?:pk_)?add_f32", body, flags=re.M), inst
        # the wide path keeps RowSink's stores -- as many 16-byte stores as k_ans_decode_scaled of the same instantiation,
        # which has ScaledSink's -- and adds 16-byte loads for the tensor words to that kernel's (the compressed words)
        (scaled,) = [b for k, b in bodies.items() if _mangled("k_ans_decode_scaled", *inst) in k]
        count = lambda op, text: len(re.findall(r"^\s+%s\b" % op, text, flags=re.M))
        assert count("global_store_dwordx4", body) == count("global_store_dwordx4", scaled) > 0, inst
        assert count("global_load_dwordx4", body) > count("global_load_dwordx4", scaled), inst


def test_the_table_row_is_present():
    text = open(os.path.join(ROOT, "dietgpu_amd", "csrc", "kernel_variants.h")).read()
    assert "X(kUpdate, k_ans_decode_update, halvesOnly, decLdsBytes(P, T, TB))" in text
    assert "X(kAccumScaled, k_ans_decode_accum_scaled, floatsOnly, decLdsBytes(P, T, TB))" in text  # the LDS of k_ans_decode_accum_scaled
    assert "return {kernel<P, T, TB>, decThreads(TB), ldsBytes, #kernel};" in text
