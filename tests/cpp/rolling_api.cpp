// Rolling-table compress through the C++ mirror (include/dietgpu_amd/GpuRollingCodec.h): three bfloat16 elements are
// compressed three times with floatCompressRolling -- counts only, then twice with ONE counts buffer as input and output
// while the data changes -- and decoded with floatDecompress.  Every round trip is bit exact, the counts after each call
// are the histogram of the exponent bytes of that call's data, and a call whose counts are its data's own writes the
// archive of plain floatCompress byte for byte.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuRollingCodec.h"

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

static uint16_t toBf16(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  return (uint16_t)((x + 0x7fffu + ((x >> 16) & 1u)) >> 16);
}

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  const std::vector<uint32_t> sizes = {3u, 4097u, 40000u};
  const uint32_t B = (uint32_t)sizes.size();
  std::mt19937 gen(13);
  std::vector<std::vector<uint16_t>> host(B);
  std::vector<const void*> in(B);
  std::vector<void*> comp(B), plain(B), out(B);
  std::vector<uint32_t> inSize(B);
  for (uint32_t b = 0; b < B; ++b) {
    host[b].resize(sizes[b]);
    void* d = nullptr;
    HIP(hipMalloc(&d, sizes[b] * 2));
    in[b] = d;
    inSize[b] = sizes[b];
    HIP(hipMalloc(&comp[b], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    HIP(hipMalloc(&plain[b], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    HIP(hipMalloc(&out[b], sizes[b] * 2));
  }
  uint32_t *compSize_dev, *plainSize_dev, *outSize_dev, *counts_dev;
  uint8_t* success_dev;
  HIP(hipMalloc((void**)&compSize_dev, B * 4));
  HIP(hipMalloc((void**)&plainSize_dev, B * 4));
  HIP(hipMalloc((void**)&outSize_dev, B * 4));
  HIP(hipMalloc((void**)&counts_dev, B * 256 * 4));
  HIP(hipMemsetAsync(counts_dev, 0xa5, B * 256 * 4, stream));  // nothing is required of what the buffer held
  HIP(hipMalloc((void**)&success_dev, B));
  ANSCodecConfig ans(10, false);
  FloatCodecConfig fc(FloatType::kBFloat16, ans, false, false);
  for (int step = 0; step < 3; ++step) {
    std::normal_distribution<float> dist(0.0f, 1.0f + 2.0f * (float)step);
    std::vector<std::vector<uint32_t>> want(B, std::vector<uint32_t>(256, 0u));
    for (uint32_t b = 0; b < B; ++b) {
      for (uint32_t i = 0; i < sizes[b]; ++i) {
        host[b][i] = toBf16(dist(gen));
        want[b][(host[b][i] >> 7) & 0xffu]++;
      }
      HIP(hipMemcpyAsync((void*)in[b], host[b].data(), sizes[b] * 2, hipMemcpyHostToDevice, stream));
    }
    floatCompressRolling(res, fc, false, B, in.data(), inSize.data(), step == 0 ? nullptr : counts_dev, counts_dev, comp.data(),
                         compSize_dev, stream);
    std::vector<const void*> compIn(comp.begin(), comp.end());
    FloatDecompressStatus st = floatDecompress(res, fc, B, compIn.data(), out.data(), inSize.data(), success_dev, outSize_dev, stream);
    EXPECT(st.error == FloatDecompressError::None);
    std::vector<uint32_t> outSize(B), compSize(B), plainSize(B), counts(B * 256);
    std::vector<uint8_t> success(B);
    if (step == 0) {
      floatCompress(res, fc, B, in.data(), inSize.data(), plain.data(), plainSize_dev, stream);
      HIP(hipMemcpyAsync(plainSize.data(), plainSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
    }
    HIP(hipMemcpyAsync(outSize.data(), outSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(compSize.data(), compSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(success.data(), success_dev, B, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(counts.data(), counts_dev, B * 256 * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipStreamSynchronize(stream));
    for (uint32_t b = 0; b < B; ++b) {
      std::vector<uint16_t> got(sizes[b]);
      HIP(hipMemcpyAsync(got.data(), out[b], sizes[b] * 2, hipMemcpyDeviceToHost, stream));
      HIP(hipStreamSynchronize(stream));
      EXPECT(success[b] == 1);
      EXPECT(outSize[b] == sizes[b]);
      EXPECT(compSize[b] > 16 && compSize[b] <= getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b]));
      EXPECT(memcmp(got.data(), host[b].data(), sizes[b] * 2) == 0);
      EXPECT(memcmp(&counts[b * 256], want[b].data(), 256 * 4) == 0);
      if (step == 0) {
        EXPECT(plainSize[b] == compSize[b]);
        std::vector<uint8_t> x(compSize[b]), y(compSize[b]);
        HIP(hipMemcpyAsync(x.data(), comp[b], compSize[b], hipMemcpyDeviceToHost, stream));
        HIP(hipMemcpyAsync(y.data(), plain[b], compSize[b], hipMemcpyDeviceToHost, stream));
        HIP(hipStreamSynchronize(stream));
        EXPECT(x == y);
      }
    }
  }
  for (uint32_t b = 0; b < B; ++b) {
    HIP(hipFree(out[b]));
    HIP(hipFree(comp[b]));
    HIP(hipFree(plain[b]));
    HIP(hipFree((void*)in[b]));
  }
  HIP(hipFree(compSize_dev));
  HIP(hipFree(plainSize_dev));
  HIP(hipFree(outSize_dev));
  HIP(hipFree(counts_dev));
  HIP(hipFree(success_dev));
  if (failures) {
    printf("rolling_api: %d FAILURES\n", failures);
    return 1;
  }
  printf("rolling_api: OK\n");
  return 0;
}
