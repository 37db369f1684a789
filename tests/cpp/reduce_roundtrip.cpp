// Decode-reduce through the C++ mirror (include/dietgpu_amd/GpuAccumulateCodec.h): three bf16 members of three sources
// each, compressed with floatCompress; floatDecompressReduce with accumulate = false and then true, compared bit for
// bit with the left-to-right float32 sum made on the host, guard words around every accumulator; then one source
// truncated: its member fails and keeps its bits, the others are summed.
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
static float add(float x, float y) {
  volatile float sum = x + y;  // one float32 add, not folded into anything
  return sum;
}
static uint32_t bitsOf(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  const std::vector<uint32_t> sizes = {1u, 4097u, 40000u};
  const uint32_t B = (uint32_t)sizes.size(), S = 3, guard = 64;
  const uint32_t kSentinel = 0xcdcdcdcdu;
  std::mt19937 gen(11);
  std::normal_distribution<float> dist(0.0f, 1.0f);
  // member-major: source s of member b at b * S + s
  std::vector<std::vector<uint16_t>> host(B * S);
  std::vector<const void*> in(B * S);
  std::vector<void*> comp(B * S);
  std::vector<uint32_t> inSize(B * S), cap(B);
  std::vector<float*> acc(B);
  for (uint32_t b = 0; b < B; ++b) {
    for (uint32_t s = 0; s < S; ++s) {
      const uint32_t k = b * S + s;
      host[k].resize(sizes[b]);
      for (auto& v : host[k]) v = (uint16_t)(bitsOf(dist(gen) * (float)(1u << (4u * s))) >> 16);
      uint16_t* d = nullptr;
      HIP(hipMalloc((void**)&d, sizes[b] * 2));
      HIP(hipMemcpyAsync(d, host[k].data(), sizes[b] * 2, hipMemcpyHostToDevice, stream));
      in[k] = d;
      inSize[k] = sizes[b];
      HIP(hipMalloc(&comp[k], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    }
    cap[b] = sizes[b];
    float* a = nullptr;
    HIP(hipMalloc((void**)&a, (sizes[b] + 2 * guard) * 4));
    HIP(hipMemsetAsync(a, 0xcd, (sizes[b] + 2 * guard) * 4, stream));
    acc[b] = a + guard;
  }
  uint32_t* compSize_dev;
  uint32_t* outSize_dev;
  uint8_t* success_dev;
  HIP(hipMalloc((void**)&compSize_dev, B * S * 4));
  HIP(hipMalloc((void**)&outSize_dev, B * 4));
  HIP(hipMalloc((void**)&success_dev, B));
  ANSCodecConfig ans(10, false);
  FloatCodecConfig fc(FloatType::kBFloat16, ans, false, false);
  floatCompress(res, fc, B * S, in.data(), inSize.data(), comp.data(), compSize_dev, stream);
  std::vector<uint32_t> compSize(B * S);
  HIP(hipMemcpyAsync(compSize.data(), compSize_dev, B * S * 4, hipMemcpyDeviceToHost, stream));
  HIP(hipStreamSynchronize(stream));
  std::vector<const void*> compIn(comp.begin(), comp.end());

  // what the accumulators must hold, kept on the host from pass to pass
  std::vector<std::vector<uint32_t>> want(B);
  for (uint32_t b = 0; b < B; ++b) want[b].assign(sizes[b], kSentinel);

  // pass 0 stores the sum of the sources, pass 1 adds them once more, pass 2 has a truncated source in member 1
  for (int pass = 0; pass < 3; ++pass) {
    std::vector<uint32_t> offered(compSize);
    if (pass == 2) offered[1 * S + 2] -= 16;
    floatDecompressReduce(res, fc, pass >= 1, B, S, compIn.data(), offered.data(), acc.data(), cap.data(), success_dev,
                          outSize_dev, stream);
    std::vector<uint32_t> outSize(B);
    std::vector<uint8_t> success(B);
    HIP(hipMemcpyAsync(outSize.data(), outSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(success.data(), success_dev, B, hipMemcpyDeviceToHost, stream));
    for (uint32_t b = 0; b < B; ++b) {
      std::vector<uint32_t> got(sizes[b] + 2 * guard);
      HIP(hipMemcpyAsync(got.data(), acc[b] - guard, got.size() * 4, hipMemcpyDeviceToHost, stream));
      HIP(hipStreamSynchronize(stream));
      const bool fails = pass == 2 && b == 1;
      EXPECT(success[b] == (fails ? 0 : 1));
      EXPECT(outSize[b] == sizes[b]);
      uint32_t bad = 0;
      for (uint32_t i = 0; i < sizes[b]; ++i) {
        if (!fails) {
          float sum = 0.0f;
          for (uint32_t s = 0; s < S; ++s) {
            const float w = widen(host[b * S + s][i]);
            if (s == 0 && pass == 0) {
              sum = w;  // stored as it is
            } else {
              float before;
              memcpy(&before, &want[b][i], 4);
              sum = add(s == 0 ? before : sum, w);
            }
          }
          want[b][i] = bitsOf(sum);
        }
        bad += want[b][i] != got[guard + i];
      }
      EXPECT(bad == 0);
      for (uint32_t g = 0; g < guard; ++g) {
        EXPECT(got[g] == kSentinel);
        EXPECT(got[guard + sizes[b] + g] == kSentinel);
      }
    }
  }
  for (uint32_t b = 0; b < B; ++b) HIP(hipFree(acc[b] - guard));
  for (uint32_t k = 0; k < B * S; ++k) {
    HIP(hipFree(comp[k]));
    HIP(hipFree((void*)in[k]));
  }
  HIP(hipFree(compSize_dev));
  HIP(hipFree(outSize_dev));
  HIP(hipFree(success_dev));
  if (failures) {
    printf("reduce_roundtrip: %d FAILURES\n", failures);
    return 1;
  }
  printf("reduce_roundtrip: OK\n");
  return 0;
}
