"""The stochastic cast-compress wrapper of the dietgpu:: C++ mirror (include/dietgpu_amd/GpuStochasticCodec.h)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "stochastic_api.cpp")


def test_stochastic_header_is_plain_host_cxx17():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), SRC])
    assert "floatCompressStochastic(" in open(SRC).read()


@pytest.mark.gpu
def test_cpp_stochastic_api(tmp_path):
    exe = str(tmp_path / "stochastic_api")
    lib = os.path.join(ROOT, "dietgpu_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-L" + lib, "-ldietgpu_amd",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "stochastic_api: OK" in out.stdout
