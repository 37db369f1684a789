"""Work planning (csrc/work_plan.h) on the CPU: tests/cpp/plan_dump.cpp prints every launch group and the whole work
vector of a fixed table of batches -- rectangles, ragged batches, size classes and their fall-backs, under every setting
of the two test hooks -- and the output must be tests/plan_dump.expected, which was recorded from the planning functions
as they stood inside capi.hip (RaggedPlan / EncodeClass / DecodeClass) before they were unified.  Built with the address
and undefined-behaviour sanitizers: plain host C++, no HIP."""
import difflib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "plan_dump.cpp")
EXPECTED = os.path.join(ROOT, "tests", "plan_dump.expected")


def test_planner_headers_need_no_rocm():
    for name in ("work_plan.h", "plan_constants.h"):
        subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "dietgpu_amd", "csrc"), "-x", "c++", "-"], input=f'#include "{name}"\n', text=True, check=True)


def test_plans_are_the_recorded_ones(tmp_path):
    exe = str(tmp_path / "plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
    expected = open(EXPECTED).read()
    if out.stdout != expected:
        diff = list(difflib.unified_diff(expected.splitlines(), out.stdout.splitlines(), "expected", "plan_dump", lineterm="", n=2))
        raise AssertionError("work plans changed:\n" + "\n".join(diff[:80]))
