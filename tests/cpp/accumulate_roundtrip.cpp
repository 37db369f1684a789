// Decode-accumulate through the C++ mirror (include/dietgpu_amd/GpuAccumulateCodec.h): three bf16 elements compressed
// with floatCompress, floatDecompressAccumulate with accumulate = false and then true, compared bit for bit with a sum
// made on the host, guard words around every accumulator.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuAccumulateCodec.h"

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

static float widen(uint16_t bf16) {
  const uint32_t bits = (uint32_t)bf16 << 16;
  float f;
  memcpy(&f, &bits, 4);
  return f;
}

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  const std::vector<uint32_t> sizes = {1u, 4097u, 40000u};
  const uint32_t B = (uint32_t)sizes.size(), guard = 64;
  const uint32_t kSentinel = 0xcdcdcdcdu;
  std::mt19937 gen(7);
  std::normal_distribution<float> dist(0.0f, 1.0f);
  std::vector<std::vector<uint16_t>> host(B);
  std::vector<const void*> in(B);
  std::vector<void*> comp(B);
  std::vector<float*> acc(B);
  std::vector<uint32_t> inSize(B), cap(B);
  for (uint32_t b = 0; b < B; ++b) {
    host[b].resize(sizes[b]);
    for (auto& v : host[b]) {
      const float f = dist(gen);
      uint32_t bits;
      memcpy(&bits, &f, 4);
      v = (uint16_t)(bits >> 16);
    }
    uint16_t* d = nullptr;
    HIP(hipMalloc((void**)&d, sizes[b] * 2));
    HIP(hipMemcpyAsync(d, host[b].data(), sizes[b] * 2, hipMemcpyHostToDevice, stream));
    in[b] = d;
    inSize[b] = sizes[b];
    cap[b] = sizes[b];
    HIP(hipMalloc(&comp[b], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    float* a = nullptr;
    HIP(hipMalloc((void**)&a, (sizes[b] + 2 * guard) * 4));
    HIP(hipMemsetAsync(a, 0xcd, (sizes[b] + 2 * guard) * 4, stream));
    acc[b] = a + guard;
  }
  uint32_t* compSize_dev;
  uint32_t* outSize_dev;
  uint8_t* success_dev;
  HIP(hipMalloc((void**)&compSize_dev, B * 4));
  HIP(hipMalloc((void**)&outSize_dev, B * 4));
  HIP(hipMalloc((void**)&success_dev, B));
  ANSCodecConfig ans(10, false);
  FloatCodecConfig fc(FloatType::kBFloat16, ans, false, false);
  floatCompress(res, fc, B, in.data(), inSize.data(), comp.data(), compSize_dev, stream);
  std::vector<uint32_t> compSize(B);
  HIP(hipMemcpyAsync(compSize.data(), compSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
  HIP(hipStreamSynchronize(stream));
  std::vector<const void*> compIn(comp.begin(), comp.end());

  // pass 0 stores the widened words, pass 1 adds them once more
  for (int pass = 0; pass < 2; ++pass) {
    floatDecompressAccumulate(res, fc, pass == 1, B, compIn.data(), compSize.data(), acc.data(), cap.data(), success_dev,
                              outSize_dev, stream);
    std::vector<uint32_t> outSize(B);
    std::vector<uint8_t> success(B);
    HIP(hipMemcpyAsync(outSize.data(), outSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(success.data(), success_dev, B, hipMemcpyDeviceToHost, stream));
    for (uint32_t b = 0; b < B; ++b) {
      std::vector<uint32_t> got(sizes[b] + 2 * guard);
      HIP(hipMemcpyAsync(got.data(), acc[b] - guard, got.size() * 4, hipMemcpyDeviceToHost, stream));
      HIP(hipStreamSynchronize(stream));
      EXPECT(success[b] == 1);
      EXPECT(outSize[b] == sizes[b]);
      uint32_t bad = 0;
      for (uint32_t i = 0; i < sizes[b]; ++i) {
        const float w = widen(host[b][i]);
        volatile float sum = w + w;  // one float32 add, not folded into anything
        const float want = pass == 0 ? w : (float)sum;
        uint32_t bits;
        memcpy(&bits, &want, 4);
        bad += bits != got[guard + i];
      }
      EXPECT(bad == 0);
      for (uint32_t g = 0; g < guard; ++g) {
        EXPECT(got[g] == kSentinel);
        EXPECT(got[guard + sizes[b] + g] == kSentinel);
      }
    }
  }
  for (uint32_t b = 0; b < B; ++b) {
    HIP(hipFree(acc[b] - guard));
    HIP(hipFree(comp[b]));
    HIP(hipFree((void*)in[b]));
  }
  HIP(hipFree(compSize_dev));
  HIP(hipFree(outSize_dev));
  HIP(hipFree(success_dev));
  if (failures) {
    printf("accumulate_roundtrip: %d FAILURES\n", failures);
    return 1;
  }
  printf("accumulate_roundtrip: OK\n");
  return 0;
}
