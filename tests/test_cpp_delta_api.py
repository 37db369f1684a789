"""The XOR-delta wrappers of the dietgpu:: C++ mirror (include/dietgpu_amd/GpuDeltaCodec.h)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "delta_api.cpp")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), SRC]


def test_delta_header_is_plain_host_cxx17():
    subprocess.check_call(["g++", "-fsyntax-only"] + FLAGS)


@pytest.mark.gpu
def test_cpp_delta_api(tmp_path):
    exe, lib = str(tmp_path / "delta_api"), os.path.join(ROOT, "dietgpu_amd", "lib")
    subprocess.check_call(["g++", "-O1"] + FLAGS + ["-o", exe, "-L" + lib, "-ldietgpu_amd", "-L/opt/rocm/lib", "-lamdhip64",
                                                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "delta_api: OK" in out.stdout, out.stdout + out.stderr
