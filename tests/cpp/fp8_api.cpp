// FP8 archives through the C++ mirror (include/dietgpu_amd/GpuFp8Codec.h): one tensor through fp8CompressCast (e5m2,
// factor 64) and fp8DecompressAccumulate (factor 1/64, stored).  The values are multiples of 2^-10 with two significant
// bits, which e5m2 holds exactly: the round trip returns them bit for bit.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuFp8Codec.h"

using namespace dietgpu;

#define HIP(x) DIETGPU_HIP_VERIFY(x)

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  const uint32_t n = 70001u;
  std::mt19937 gen(29);
  std::vector<float> host(n), back(n);
  for (uint32_t i = 0; i < n; ++i) host[i] = (float)((int)(gen() % 7u) - 3) * (float)(1u << (gen() % 4u)) / 1024.0f;
  void *in, *acc, *comp;
  uint32_t* size_dev;  // archive size, decoded size
  uint8_t* ok_dev;
  HIP(hipMalloc(&in, n * 4));
  HIP(hipMalloc(&acc, n * 4));
  HIP(hipMemcpy(in, host.data(), n * 4, hipMemcpyHostToDevice));
  HIP(hipMalloc(&comp, getMaxCompressedSize(n)));
  HIP(hipMalloc((void**)&size_dev, 8));
  HIP(hipMalloc((void**)&ok_dev, 1));
  const ANSCodecConfig config(10, false);
  const void* src = in;
  fp8CompressCast(config, Fp8Type::kE5M2, 1, &src, &n, 64.0f, nullptr, false, &comp, size_dev, stream);
  uint32_t got[2] = {0, 0};
  uint8_t ok = 0;
  HIP(hipMemcpyAsync(got, size_dev, 4, hipMemcpyDeviceToHost, stream));
  HIP(hipStreamSynchronize(stream));
  const void* archive = comp;
  fp8DecompressAccumulate(config, Fp8Type::kE5M2, false, 1, &archive, &got[0], 1.0f / 64.0f, nullptr, false, &acc, &n, ok_dev, size_dev + 1, stream);
  HIP(hipMemcpyAsync(&ok, ok_dev, 1, hipMemcpyDeviceToHost, stream));
  HIP(hipMemcpyAsync(got, size_dev, 8, hipMemcpyDeviceToHost, stream));
  HIP(hipMemcpyAsync(back.data(), acc, n * 4, hipMemcpyDeviceToHost, stream));
  HIP(hipStreamSynchronize(stream));
  const bool pass = got[0] != 0 && got[0] < n && ok == 1 && got[1] == n && memcmp(back.data(), host.data(), n * 4) == 0;
  printf(pass ? "fp8_api: OK\n" : "fp8_api: FAILED (archive %u bytes, ok %u, size %u)\n", got[0], ok, got[1]);
  return pass ? 0 : 1;
}
