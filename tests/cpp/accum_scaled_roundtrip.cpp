// Scaled decode-accumulate through the C++ mirror (include/dietgpu_amd/GpuAccumulateCodec.h): three bf16 elements
// compressed with floatCompress, decoded plainly with floatDecompress, and decoded with floatDecompressAccumulateScaled --
// a host factor, one device factor, one device factor per element; stored and added -- compared bit for bit with the
// plain decode followed by the arithmetic on the host: one float32 multiply and one float32 add, two roundings.  Guard
// words around every accumulator.
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

// (the inputs, factors and accumulators are finite: nothing is a NaN)
static uint32_t onHost(uint16_t bf16, float factor, bool accumulate, float acc) {
  const uint32_t wide = (uint32_t)bf16 << 16;
  float w;
  memcpy(&w, &wide, 4);
  volatile float product = w * factor;  // one float32 multiply, rounded on its own
  volatile float sum = accumulate ? acc + product : product;
  const float s = sum;
  uint32_t x;
  memcpy(&x, &s, 4);
  return x;
}

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  const std::vector<uint32_t> sizes = {1u, 4097u, 70000u};
  const uint32_t B = (uint32_t)sizes.size(), guard = 64;
  const uint32_t kSentinel = 0xcdcdcdcdu;
  std::mt19937 gen(13);
  std::normal_distribution<float> dist(0.0f, 1.0f);
  std::vector<const void*> in(B);
  std::vector<void*> comp(B), plain(B);
  std::vector<float*> out(B);
  std::vector<uint32_t> inSize(B), cap(B);
  std::vector<std::vector<float>> start(B);
  for (uint32_t b = 0; b < B; ++b) {
    std::vector<uint16_t> host(sizes[b]);
    start[b].resize(sizes[b]);
    for (uint32_t i = 0; i < sizes[b]; ++i) {
      const float f = dist(gen);
      uint32_t bits;
      memcpy(&bits, &f, 4);
      host[i] = (uint16_t)(bits >> 16);
      start[b][i] = 3.0f * dist(gen);
    }
    uint16_t* d = nullptr;
    HIP(hipMalloc((void**)&d, sizes[b] * 2));
    HIP(hipMemcpyAsync(d, host.data(), sizes[b] * 2, hipMemcpyHostToDevice, stream));
    HIP(hipStreamSynchronize(stream));
    in[b] = d;
    inSize[b] = sizes[b];
    cap[b] = sizes[b];
    HIP(hipMalloc(&comp[b], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    HIP(hipMalloc(&plain[b], sizes[b] * 2));
    float* o = nullptr;
    HIP(hipMalloc((void**)&o, (sizes[b] + 2 * guard) * 4));
    out[b] = o + guard;
  }
  uint32_t* compSize_dev;
  uint32_t* outSize_dev;
  uint8_t* success_dev;
  float* factors_dev;
  HIP(hipMalloc((void**)&compSize_dev, B * 4));
  HIP(hipMalloc((void**)&outSize_dev, B * 4));
  HIP(hipMalloc((void**)&success_dev, B));
  HIP(hipMalloc((void**)&factors_dev, B * 4));
  ANSCodecConfig ans(10, false);
  FloatCodecConfig fc(FloatType::kBFloat16, ans, false, false);
  floatCompress(res, fc, B, in.data(), inSize.data(), comp.data(), compSize_dev, stream);
  std::vector<uint32_t> compSize(B);
  HIP(hipMemcpyAsync(compSize.data(), compSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
  HIP(hipStreamSynchronize(stream));
  std::vector<const void*> compIn(comp.begin(), comp.end());

  // the plain decode: what the host arithmetic starts from
  floatDecompress(res, fc, B, compIn.data(), plain.data(), cap.data(), success_dev, outSize_dev, stream);
  std::vector<std::vector<uint16_t>> words(B);
  for (uint32_t b = 0; b < B; ++b) {
    words[b].resize(sizes[b]);
    HIP(hipMemcpyAsync(words[b].data(), plain[b], sizes[b] * 2, hipMemcpyDeviceToHost, stream));
  }
  HIP(hipStreamSynchronize(stream));

  const float third = 1.0f / 3.0f;
  const std::vector<float> perMember = {-1.5f, third, 3.0e38f};
  // pass 0: the host float; pass 1: one device float; pass 2: one device float per element -- each stored, then added
  for (int pass = 0; pass < 6; ++pass) {
    const int how = pass % 3;
    const bool accumulate = pass >= 3;
    for (uint32_t b = 0; b < B; ++b) {
      HIP(hipMemsetAsync(out[b] - guard, 0xcd, (sizes[b] + 2 * guard) * 4, stream));
      if (accumulate) HIP(hipMemcpyAsync(out[b], start[b].data(), sizes[b] * 4, hipMemcpyHostToDevice, stream));
    }
    std::vector<float> factor(B, how == 0 ? third : -1.5f);
    if (how == 2) factor = perMember;
    HIP(hipMemcpyAsync(factors_dev, factor.data(), B * 4, hipMemcpyHostToDevice, stream));
    HIP(hipStreamSynchronize(stream));
    floatDecompressAccumulateScaled(res, fc, accumulate, B, compIn.data(), compSize.data(), out.data(), cap.data(),
                                    how == 0 ? third : 1.0f, how == 0 ? nullptr : factors_dev, how == 2 ? 1u : 0u, success_dev,
                                    outSize_dev, stream);
    std::vector<uint32_t> outSize(B);
    std::vector<uint8_t> success(B);
    HIP(hipMemcpyAsync(outSize.data(), outSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(success.data(), success_dev, B, hipMemcpyDeviceToHost, stream));
    for (uint32_t b = 0; b < B; ++b) {
      std::vector<uint32_t> got(sizes[b] + 2 * guard);
      HIP(hipMemcpyAsync(got.data(), out[b] - guard, got.size() * 4, hipMemcpyDeviceToHost, stream));
      HIP(hipStreamSynchronize(stream));
      EXPECT(success[b] == 1);
      EXPECT(outSize[b] == sizes[b]);
      uint32_t bad = 0;
      for (uint32_t i = 0; i < sizes[b]; ++i) bad += onHost(words[b][i], factor[b], accumulate, start[b][i]) != got[guard + i];
      EXPECT(bad == 0);
      for (uint32_t g = 0; g < guard; ++g) {
        EXPECT(got[g] == kSentinel);
        EXPECT(got[guard + sizes[b] + g] == kSentinel);
      }
    }
  }
  for (uint32_t b = 0; b < B; ++b) {
    HIP(hipFree(out[b] - guard));
    HIP(hipFree(plain[b]));
    HIP(hipFree(comp[b]));
    HIP(hipFree((void*)in[b]));
  }
  HIP(hipFree(compSize_dev));
  HIP(hipFree(outSize_dev));
  HIP(hipFree(success_dev));
  HIP(hipFree(factors_dev));
  if (failures) {
    printf("accum_scaled_roundtrip: %d FAILURES\n", failures);
    return 1;
  }
  printf("accum_scaled_roundtrip: OK\n");
  return 0;
}
