// Decode-update through the C++ mirror (include/dietgpu_amd/GpuUpdateCodec.h): three bf16 elements compressed with
// floatCompress and applied to prefilled bf16 tensors with floatDecompressUpdate -- a host factor and seed, then device
// factors per element and a device seed, with and without accumulate -- compared bit for bit with the C call
// dgpu_float_decode_update given the same arguments on a second set of tensors.  Guard words around every tensor.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuUpdateCodec.h"

using namespace dietgpu;

#define HIP(x) DIETGPU_HIP_VERIFY(x)

static int failures = 0;
#define EXPECT(c)                                           \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c);  \
      ++failures;                                           \
    }                                                       \
  } while (0)

static std::vector<uint16_t> randomBf16(std::mt19937& gen, uint32_t n) {
  std::normal_distribution<float> dist(0.0f, 1.0f);
  std::vector<uint16_t> host(n);
  for (auto& v : host) {
    const float f = dist(gen);
    uint32_t bits;
    memcpy(&bits, &f, 4);
    v = (uint16_t)(bits >> 16);
  }
  return host;
}

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  const std::vector<uint32_t> sizes = {1u, 4097u, 70000u};
  const uint32_t B = (uint32_t)sizes.size(), guard = 64;
  const uint16_t kSentinel = 0xcdcdu;
  std::mt19937 gen(13);
  std::vector<const void*> in(B);
  std::vector<void*> comp(B), mirror(B), direct(B);
  std::vector<std::vector<uint16_t>> start(B);
  std::vector<uint32_t> inSize(B), cap(B);
  for (uint32_t b = 0; b < B; ++b) {
    const std::vector<uint16_t> host = randomBf16(gen, sizes[b]);
    start[b] = randomBf16(gen, sizes[b]);
    uint16_t* d = nullptr;
    HIP(hipMalloc((void**)&d, sizes[b] * 2));
    HIP(hipMemcpyAsync(d, host.data(), sizes[b] * 2, hipMemcpyHostToDevice, stream));
    HIP(hipStreamSynchronize(stream));
    in[b] = d;
    inSize[b] = sizes[b];
    cap[b] = sizes[b];
    HIP(hipMalloc(&comp[b], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    uint16_t* o = nullptr;
    HIP(hipMalloc((void**)&o, (sizes[b] + 2 * guard) * 2));
    mirror[b] = o + guard;
    HIP(hipMalloc((void**)&o, (sizes[b] + 2 * guard) * 2));
    direct[b] = o + guard;
  }
  uint32_t* compSize_dev;
  uint32_t* outSize_dev;
  uint8_t* success_dev;
  float* factors_dev;
  uint64_t* seed_dev;
  HIP(hipMalloc((void**)&compSize_dev, B * 4));
  HIP(hipMalloc((void**)&outSize_dev, B * 4));
  HIP(hipMalloc((void**)&success_dev, B));
  HIP(hipMalloc((void**)&factors_dev, B * 4));
  HIP(hipMalloc((void**)&seed_dev, 8));
  ANSCodecConfig ans(10, false);
  FloatCodecConfig fc(FloatType::kBFloat16, ans, false, false);
  floatCompress(res, fc, B, in.data(), inSize.data(), comp.data(), compSize_dev, stream);
  std::vector<uint32_t> compSize(B);
  HIP(hipMemcpyAsync(compSize.data(), compSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
  HIP(hipStreamSynchronize(stream));
  std::vector<const void*> compIn(comp.begin(), comp.end());

  const std::vector<float> perMember = {-1.5f, 1.0f / 3.0f, -0.25f};
  const uint64_t seed = 0x0123456789abcdefull;
  HIP(hipMemcpyAsync(factors_dev, perMember.data(), B * 4, hipMemcpyHostToDevice, stream));
  HIP(hipMemcpyAsync(seed_dev, &seed, 8, hipMemcpyHostToDevice, stream));
  HIP(hipStreamSynchronize(stream));
  // pass 0 / 1: host factor and seed, accumulate off / on; pass 2 / 3: device factors and seed, accumulate off / on
  for (int pass = 0; pass < 4; ++pass) {
    const bool accumulate = (pass & 1) != 0, onDevice = pass >= 2;
    for (auto* set : {&mirror, &direct}) {
      for (uint32_t b = 0; b < B; ++b) {
        HIP(hipMemsetAsync((uint16_t*)(*set)[b] - guard, 0xcd, (sizes[b] + 2 * guard) * 2, stream));
        HIP(hipMemcpyAsync((*set)[b], start[b].data(), sizes[b] * 2, hipMemcpyHostToDevice, stream));
      }
    }
    HIP(hipStreamSynchronize(stream));
    floatDecompressUpdate(fc, accumulate, B, compIn.data(), compSize.data(), mirror.data(), cap.data(), -0.25f,
                          onDevice ? factors_dev : nullptr, onDevice ? 1u : 0u, seed + 1, onDevice ? seed_dev : nullptr, 5u, success_dev,
                          outSize_dev, stream);
    std::vector<uint32_t> outSize(B);
    std::vector<uint8_t> success(B);
    HIP(hipMemcpyAsync(outSize.data(), outSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(success.data(), success_dev, B, hipMemcpyDeviceToHost, stream));
    HIP(hipStreamSynchronize(stream));
    const int rc = dgpu_float_decode_update(DGPU_BFLOAT16, 10, accumulate ? 1 : 0, B, compIn.data(), compSize.data(), direct.data(),
                                            cap.data(), -0.25f, onDevice ? factors_dev : nullptr, onDevice ? 1u : 0u, seed + 1,
                                            onDevice ? seed_dev : nullptr, 5u, nullptr, nullptr, stream);
    EXPECT(rc == 0);
    for (uint32_t b = 0; b < B; ++b) {
      std::vector<uint16_t> got(sizes[b] + 2 * guard), want(sizes[b] + 2 * guard);
      HIP(hipMemcpyAsync(got.data(), (uint16_t*)mirror[b] - guard, got.size() * 2, hipMemcpyDeviceToHost, stream));
      HIP(hipMemcpyAsync(want.data(), (uint16_t*)direct[b] - guard, want.size() * 2, hipMemcpyDeviceToHost, stream));
      HIP(hipStreamSynchronize(stream));
      EXPECT(success[b] == 1);
      EXPECT(outSize[b] == sizes[b]);
      EXPECT(got == want);
      uint32_t moved = 0;
      for (uint32_t i = 0; i < sizes[b]; ++i) moved += got[guard + i] != start[b][i];
      EXPECT(sizes[b] < 64u || moved > sizes[b] / 2u);  // the call did write the tensor
      for (uint32_t g = 0; g < guard; ++g) {
        EXPECT(got[g] == kSentinel);
        EXPECT(got[guard + sizes[b] + g] == kSentinel);
      }
    }
  }
  for (uint32_t b = 0; b < B; ++b) {
    HIP(hipFree((uint16_t*)mirror[b] - guard));
    HIP(hipFree((uint16_t*)direct[b] - guard));
    HIP(hipFree(comp[b]));
    HIP(hipFree((void*)in[b]));
  }
  HIP(hipFree(compSize_dev));
  HIP(hipFree(outSize_dev));
  HIP(hipFree(success_dev));
  HIP(hipFree(factors_dev));
  HIP(hipFree(seed_dev));
  if (failures) {
    printf("update_api: %d FAILURES\n", failures);
    return 1;
  }
  printf("update_api: OK\n");
  return 0;
}
