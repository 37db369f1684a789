"""The feedback cast-compress wrapper of the dietgpu:: C++ mirror (include/dietgpu_amd/GpuFeedbackCodec.h)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "feedback_roundtrip.cpp")


def test_feedback_header_is_plain_host_cxx17():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), SRC])
    assert "floatCompressFeedback(" in open(SRC).read()


@pytest.mark.gpu
def test_cpp_feedback_roundtrip(tmp_path):
    exe = str(tmp_path / "feedback_roundtrip")
    lib = os.path.join(ROOT, "dietgpu_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-L" + lib, "-ldietgpu_amd",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "feedback_roundtrip: OK" in out.stdout
