"""Registers and LDS of the counting form of k_ans_encode (no GPU needed: hipcc cross-compiles).

The counting encoder carries, beside everything the plain encoder holds across the row loop, the LDS address of the
lane's bin column, and adds one ds_add per row.  It is held to what the plain form of the same geometry compiles to: no
scratch, no AGPRs, and compiler-reported waves per SIMD not below the plain form's.  The bins bring the 8-block 16-bit
forms to 32.1 KiB (bf16) / 36.1 KiB (fp16) of LDS: four workgroups per CU (a static_assert here and in
kernels_encode.h).  Counting and plain forms are instantiated in one translation unit of their own: seconds, not the
minutes of the whole library."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [("10", "kBFloat16", "kBlocksPerTile"), ("11", "kFloat16", "kBlocksPerTile"),
         ("10", "kBFloat16 | kCastSource", "kBlocksPerSmallTile"), ("10", "kBFloat16", "kBlocksPerTinyTile")]
SOURCE = """
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels_encode.h"
namespace dgpu {
%s
static_assert(4u * encCountLdsBytes(10, kBFloat16, kBlocksPerTile) <= 160u * 1024u, "four workgroups per CU");
static_assert(4u * encCountLdsBytes(11, kFloat16, kBlocksPerTile) <= 160u * 1024u, "four workgroups per CU");
static_assert(4u * encCountLdsBytes(11, kFloat16 | kCastSource, kBlocksPerTile) <= 160u * 1024u, "four workgroups per CU");
}
""" % "\n".join(
    "template __global__ void k_ans_encode<%s, %s, true, %s, true, false, %s>(EncodeArgs);" % (p, ft, tb, count)
    for p, ft, tb in FORMS for count in ("false", "true"))


def _resources(tmp_path):
    src = tmp_path / "rolling_kernels.hip"
    src.write_text(SOURCE)
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "dietgpu_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "rolling_kernels.o"), str(src)], capture_output=True, text=True)
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
    return {k: v for k, v in kernels.items() if "k_ans_encode" in k}


def test_counting_encoders_keep_the_plain_forms_occupancy(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on PATH")
    enc = _resources(tmp_path)
    assert len(enc) == 2 * len(FORMS), list(enc)
    # Itanium mangling: the last template argument (kCount) is Lb0E / Lb1E right before the closing E of the list
    counting = {k: v for k, v in enc.items() if re.search(r"Lb1EEEv", k)}
    plain = {k: v for k, v in enc.items() if re.search(r"Lb0EEEv", k)}
    assert len(counting) == len(plain) == len(FORMS), list(enc)
    for name, r in counting.items():
        twin = plain[name.replace("Lb1EEEv", "Lb0EEEv")]
        print(name, "vgpr", r["VGPRs"], "/", twin["VGPRs"], "occupancy", r["Occupancy [waves/SIMD]"], "/", twin["Occupancy [waves/SIMD]"],
              "lds", r["LDS Size [bytes/block]"], "/", twin["LDS Size [bytes/block]"])
        assert int(r["AGPRs"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(twin["ScratchSize [bytes/lane]"]) == 0, (name, twin)
        assert int(r["Occupancy [waves/SIMD]"]) >= int(twin["Occupancy [waves/SIMD]"]), (name, r, twin)
