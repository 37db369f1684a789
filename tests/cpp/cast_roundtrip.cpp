// Cast-compress through the C++ mirror (include/dietgpu_amd/GpuCastCodec.h): three float32 elements compressed into
// bfloat16 archives with floatCompressCast and decoded with floatDecompress; the result equals the rounding made on the
// host (round to nearest even on the bits, NaN to the canonical quiet NaN), and the inputs are unchanged.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuCastCodec.h"

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

static uint16_t roundToBf16(uint32_t x) {
  if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)(((x >> 16) & 0x8000u) | 0x7fc0u);
  return (uint16_t)(((uint64_t)x + 0x7fffu + ((x >> 16) & 1u)) >> 16);
}

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  const std::vector<uint32_t> sizes = {3u, 4097u, 40000u};
  const uint32_t B = (uint32_t)sizes.size();
  std::mt19937 gen(11);
  std::normal_distribution<float> dist(0.0f, 1.0f);
  std::vector<std::vector<uint32_t>> host(B);
  std::vector<const float*> in(B);
  std::vector<void*> comp(B), out(B);
  std::vector<uint32_t> inSize(B);
  for (uint32_t b = 0; b < B; ++b) {
    host[b].resize(sizes[b]);
    for (uint32_t i = 0; i < sizes[b]; ++i) {
      const float f = dist(gen);
      memcpy(&host[b][i], &f, 4);
      if (i % 97 == 5) host[b][i] = 0x3fffffffu;   // carries into the next exponent
      if (i % 101 == 7) host[b][i] = 0x7f800001u;  // a NaN whose payload is in the low half only
      if (i % 103 == 9) host[b][i] = 0x00008001u;  // a float32 denormal
    }
    float* d = nullptr;
    HIP(hipMalloc((void**)&d, sizes[b] * 4));
    HIP(hipMemcpyAsync(d, host[b].data(), sizes[b] * 4, hipMemcpyHostToDevice, stream));
    in[b] = d;
    inSize[b] = sizes[b];
    HIP(hipMalloc(&comp[b], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    HIP(hipMalloc(&out[b], sizes[b] * 2));
  }
  uint32_t* compSize_dev;
  uint32_t* outSize_dev;
  uint8_t* success_dev;
  HIP(hipMalloc((void**)&compSize_dev, B * 4));
  HIP(hipMalloc((void**)&outSize_dev, B * 4));
  HIP(hipMalloc((void**)&success_dev, B));
  ANSCodecConfig ans(10, false);
  FloatCodecConfig fc(FloatType::kBFloat16, ans, false, false);
  floatCompressCast(res, fc, B, in.data(), inSize.data(), comp.data(), compSize_dev, stream);
  std::vector<const void*> compIn(comp.begin(), comp.end());
  FloatDecompressStatus st = floatDecompress(res, fc, B, compIn.data(), out.data(), inSize.data(), success_dev, outSize_dev, stream);
  EXPECT(st.error == FloatDecompressError::None);
  std::vector<uint32_t> outSize(B), compSize(B);
  std::vector<uint8_t> success(B);
  HIP(hipMemcpyAsync(outSize.data(), outSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
  HIP(hipMemcpyAsync(compSize.data(), compSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
  HIP(hipMemcpyAsync(success.data(), success_dev, B, hipMemcpyDeviceToHost, stream));
  for (uint32_t b = 0; b < B; ++b) {
    std::vector<uint16_t> got(sizes[b]);
    std::vector<uint32_t> src(sizes[b]);
    HIP(hipMemcpyAsync(got.data(), out[b], sizes[b] * 2, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(src.data(), in[b], sizes[b] * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipStreamSynchronize(stream));
    EXPECT(success[b] == 1);
    EXPECT(outSize[b] == sizes[b]);
    EXPECT(compSize[b] > 16 && compSize[b] <= getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b]));
    uint32_t bad = 0, changed = 0;
    for (uint32_t i = 0; i < sizes[b]; ++i) {
      bad += got[i] != roundToBf16(host[b][i]);
      changed += src[i] != host[b][i];
    }
    EXPECT(bad == 0);
    EXPECT(changed == 0);
  }
  for (uint32_t b = 0; b < B; ++b) {
    HIP(hipFree(out[b]));
    HIP(hipFree(comp[b]));
    HIP(hipFree((void*)in[b]));
  }
  HIP(hipFree(compSize_dev));
  HIP(hipFree(outSize_dev));
  HIP(hipFree(success_dev));
  if (failures) {
    printf("cast_roundtrip: %d FAILURES\n", failures);
    return 1;
  }
  printf("cast_roundtrip: OK\n");
  return 0;
}
