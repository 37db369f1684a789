// XOR-delta archives through the C++ mirror (include/dietgpu_amd/GpuDeltaCodec.h): one round trip of one tensor --
// ansEncodeBatchDelta, then ansDecodeBatchDelta in place into a copy of the base.
#include <cstdio>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuDeltaCodec.h"

using namespace dietgpu;

#define HIP(x) DIETGPU_HIP_VERIFY(x)

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  const uint32_t n = 70001u;
  std::mt19937 gen(23);
  std::vector<uint8_t> hostIn, hostBase, back(n);
  for (uint32_t i = 0; i < n; ++i) {
    hostBase.push_back((uint8_t)gen());
    hostIn.push_back((gen() % 4u) ? hostBase[i] : (uint8_t)(hostBase[i] + 1u));  // a quarter of the bytes moved
  }
  auto upload = [&](const std::vector<uint8_t>& h) {
    void* p;
    HIP(hipMalloc(&p, n));
    HIP(hipMemcpy(p, h.data(), n, hipMemcpyHostToDevice));
    return p;
  };
  const void *in = upload(hostIn), *base = upload(hostBase);
  void *work = upload(hostBase), *comp;
  uint32_t* size_dev;  // archive size, decoded size
  uint8_t* ok_dev;
  HIP(hipMalloc(&comp, getMaxCompressedSize(n)));
  HIP(hipMalloc((void**)&size_dev, 8));
  HIP(hipMalloc((void**)&ok_dev, 1));
  const ANSCodecConfig config(10, false);
  ansEncodeBatchDelta(config, 1, &in, &base, &n, &comp, size_dev, stream);
  uint32_t got[2] = {0, 0};
  uint8_t ok = 0;
  HIP(hipMemcpyAsync(got, size_dev, 4, hipMemcpyDeviceToHost, stream));
  HIP(hipStreamSynchronize(stream));
  const void *archive = comp, *workBase = work;  // in place: the copy of the base becomes the tensor
  ansDecodeBatchDelta(config, 1, &archive, &got[0], &workBase, &work, &n, ok_dev, size_dev + 1, stream);
  HIP(hipMemcpyAsync(&ok, ok_dev, 1, hipMemcpyDeviceToHost, stream));
  HIP(hipMemcpyAsync(got, size_dev, 8, hipMemcpyDeviceToHost, stream));
  HIP(hipMemcpyAsync(back.data(), work, n, hipMemcpyDeviceToHost, stream));
  HIP(hipStreamSynchronize(stream));
  const bool pass = got[0] != 0 && got[0] < n && ok == 1 && got[1] == n && back == hostIn;
  printf(pass ? "delta_api: OK\n" : "delta_api: FAILED (archive %u bytes, ok %u, size %u)\n", got[0], ok, got[1]);
  return pass ? 0 : 1;
}
