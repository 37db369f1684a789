"""Registers and LDS of the stochastic form of k_ans_encode (no GPU needed: hipcc cross-compiles).

The stochastic source holds, beside what the cast source holds across the row loop, the member's key and the index of
the block's first word, and spends four mixes (two 32-bit multiplies each) per 8 words where the cast source adds a
constant.  It is held to no scratch, no AGPRs, the cast twin's LDS and at least 4 waves per SIMD -- the residency down
to which the project's own series shows the row loop indifferent; the twin's 6 is the aim.  The
cast twins are compiled in the same translation unit, so that the table shows what the random bits cost; seconds, not
the minutes of the whole library."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (probBits, archive type, blocks per tile, persistent): the six forms of tests/test_feedback_kernel_resources.py
FORMS = [("10", "kBFloat16", "kBlocksPerTile", "true"), ("10", "kBFloat16", "kBlocksPerSmallTile", "true"),
         ("10", "kBFloat16", "kBlocksPerSmallTile", "false"), ("10", "kBFloat16", "kBlocksPerTinyTile", "true"),
         ("10", "kBFloat16", "kBlocksPerTinyTile", "false"), ("11", "kFloat16", "kBlocksPerTile", "true")]
STOCHASTIC = 0x800
SOURCE = """
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels_encode.h"
namespace dgpu {
%s
}
""" % "\n".join(
    "template __global__ void k_ans_encode<%s, %s | kCastSource%s, true, %s, %s, false, false>(EncodeArgs);" % (p, ft, sr, tb, pers)
    for p, ft, tb, pers in FORMS for sr in ("", " | kStochasticSource"))


def _resources(tmp_path):
    src = tmp_path / "stochastic_kernels.hip"
    src.write_text(SOURCE)
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "dietgpu_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "stochastic_kernels.o"), str(src)], capture_output=True, text=True)
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


def test_stochastic_encoders_fit_four_waves_without_scratch(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on PATH")
    enc = _resources(tmp_path)
    assert len(enc) == 2 * len(FORMS), list(enc)
    # Itanium mangling: the second template argument is the source, Lj<archive type + 0x100 (cast) + 0x800 (stochastic)>E
    source = lambda name: int(re.search(r"k_ans_encodeILi\d+ELj(\d+)E", name).group(1))
    stochastic = {k: v for k, v in enc.items() if source(k) & STOCHASTIC}
    cast = {k: v for k, v in enc.items() if not source(k) & STOCHASTIC}
    assert len(stochastic) == len(cast) == len(FORMS), list(enc)
    for name, r in sorted(stochastic.items()):
        twin = cast[name.replace("Lj%dE" % source(name), "Lj%dE" % (source(name) & ~STOCHASTIC), 1)]
        print(name, "vgpr", r["VGPRs"], "/", twin["VGPRs"], "occupancy", r["Occupancy [waves/SIMD]"], "/", twin["Occupancy [waves/SIMD]"],
              "lds", r["LDS Size [bytes/block]"], "/", twin["LDS Size [bytes/block]"])
        assert int(r["AGPRs"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["LDS Size [bytes/block]"]) == int(twin["LDS Size [bytes/block]"]), (name, r, twin)
        assert int(r["Occupancy [waves/SIMD]"]) >= 4, (name, r)
        # the cast forms are what they were: no scratch, no AGPRs, six waves
        assert int(twin["AGPRs"]) == 0 and int(twin["ScratchSize [bytes/lane]"]) == 0 and int(twin["Occupancy [waves/SIMD]"]) >= 6, (name, twin)
