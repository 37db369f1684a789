"""The FP8 wrappers of the dietgpu:: C++ mirror (include/dietgpu_amd/GpuFp8Codec.h)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fp8_api.cpp")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), SRC]


def test_fp8_header_is_plain_host_cxx17():
    subprocess.check_call(["g++", "-fsyntax-only"] + FLAGS)


@pytest.mark.gpu
def test_cpp_fp8_api(tmp_path):
    exe, lib = str(tmp_path / "fp8_api"), os.path.join(ROOT, "dietgpu_amd", "lib")
    subprocess.check_call(["g++", "-O1"] + FLAGS + ["-o", exe, "-L" + lib, "-ldietgpu_amd", "-L/opt/rocm/lib", "-lamdhip64",
                                                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fp8_api: OK" in out.stdout, out.stdout + out.stderr
