// The mixed-source calls through the C++ mirror (include/dietgpu_amd/GpuAccumulateCodec.h, GpuReduceCompressCodec.h):
// three bf16 members of three sources each.  floatDecompressReduceMixed with the middle source of every member RAW must
// leave the bits floatDecompressReduce leaves on the archives of the same rows; floatDecompressReduceCompressMixed the
// accumulators, archive sizes and archive bytes floatDecompressReduceCompress leaves.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuAccumulateCodec.h"
#include "dietgpu_amd/GpuReduceCompressCodec.h"

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

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  const std::vector<uint32_t> sizes = {1u, 4097u, 40000u};
  const uint32_t B = (uint32_t)sizes.size(), S = 3;
  std::mt19937 gen(12);
  std::normal_distribution<float> dist(0.0f, 1.0f);
  std::vector<const void*> in(B * S);
  std::vector<void*> comp(B * S);
  std::vector<uint32_t> inSize(B * S), cap(B);
  for (uint32_t b = 0; b < B; ++b) {
    for (uint32_t s = 0; s < S; ++s) {
      const uint32_t k = b * S + s;
      std::vector<uint16_t> host(sizes[b]);
      for (auto& v : host) {
        const float f = dist(gen) * (float)(1u << (4u * s));
        uint32_t bits;
        memcpy(&bits, &f, 4);
        v = (uint16_t)(bits >> 16);
      }
      uint16_t* d = nullptr;
      HIP(hipMalloc((void**)&d, sizes[b] * 2));
      HIP(hipMemcpy(d, host.data(), sizes[b] * 2, hipMemcpyHostToDevice));
      in[k] = d;
      inSize[k] = sizes[b];
      HIP(hipMalloc(&comp[k], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    }
    cap[b] = sizes[b];
  }
  uint32_t *compSize_dev, *outSize_dev, *archSize_dev;
  uint8_t* success_dev;
  HIP(hipMalloc((void**)&compSize_dev, B * S * 4));
  HIP(hipMalloc((void**)&outSize_dev, B * 4));
  HIP(hipMalloc((void**)&archSize_dev, B * 4));
  HIP(hipMalloc((void**)&success_dev, B));
  ANSCodecConfig ans(10, false);
  FloatCodecConfig fc(FloatType::kBFloat16, ans, false, false);
  floatCompress(res, fc, B * S, in.data(), inSize.data(), comp.data(), compSize_dev, stream);
  std::vector<uint32_t> compSize(B * S);
  HIP(hipMemcpyAsync(compSize.data(), compSize_dev, B * S * 4, hipMemcpyDeviceToHost, stream));
  HIP(hipStreamSynchronize(stream));

  // the same rows twice: all archives, and the middle source of every member raw
  std::vector<const void*> plainIn(comp.begin(), comp.end()), mixedIn(plainIn);
  std::vector<uint32_t> plainBytes(compSize), mixedBytes(compSize);
  std::vector<uint8_t> kinds(B * S, 0);
  for (uint32_t b = 0; b < B; ++b) {
    mixedIn[b * S + 1] = in[b * S + 1];
    mixedBytes[b * S + 1] = sizes[b] * 2;
    kinds[b * S + 1] = 1;
  }
  // [0]: the plain call's accumulators and archives, [1]: the mixed call's
  std::vector<float*> acc[2];
  std::vector<void*> arch[2];
  for (int m = 0; m < 2; ++m) {
    acc[m].resize(B);
    arch[m].resize(B);
    for (uint32_t b = 0; b < B; ++b) {
      HIP(hipMalloc((void**)&acc[m][b], sizes[b] * 4));
      HIP(hipMemset(acc[m][b], 0x3c, sizes[b] * 4));
      HIP(hipMalloc(&arch[m][b], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    }
  }
  auto sameAccumulators = [&]() {
    for (uint32_t b = 0; b < B; ++b) {
      std::vector<uint32_t> x(sizes[b]), y(sizes[b]);
      HIP(hipMemcpy(x.data(), acc[0][b], sizes[b] * 4, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(y.data(), acc[1][b], sizes[b] * 4, hipMemcpyDeviceToHost));
      EXPECT(x == y);
    }
  };
  auto allSucceeded = [&]() {
    std::vector<uint8_t> ok(B);
    std::vector<uint32_t> words(B);
    HIP(hipMemcpy(ok.data(), success_dev, B, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(words.data(), outSize_dev, B * 4, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < B; ++b) EXPECT(ok[b] == 1 && words[b] == sizes[b]);
  };

  for (int accumulate = 0; accumulate < 2; ++accumulate) {
    floatDecompressReduce(res, fc, accumulate != 0, B, S, plainIn.data(), plainBytes.data(), acc[0].data(), cap.data(), success_dev,
                          outSize_dev, stream);
    HIP(hipStreamSynchronize(stream));
    allSucceeded();
    floatDecompressReduceMixed(res, fc, accumulate != 0, B, S, mixedIn.data(), mixedBytes.data(), kinds.data(), acc[1].data(), cap.data(),
                               success_dev, outSize_dev, stream);
    HIP(hipStreamSynchronize(stream));
    allSucceeded();
    sameAccumulators();
  }

  std::vector<uint32_t> archSize[2];
  floatDecompressReduceCompress(res, fc, true, B, S, plainIn.data(), plainBytes.data(), acc[0].data(), cap.data(), arch[0].data(),
                                success_dev, outSize_dev, archSize_dev, stream);
  HIP(hipStreamSynchronize(stream));
  allSucceeded();
  archSize[0].resize(B);
  HIP(hipMemcpy(archSize[0].data(), archSize_dev, B * 4, hipMemcpyDeviceToHost));
  floatDecompressReduceCompressMixed(res, fc, true, B, S, mixedIn.data(), mixedBytes.data(), kinds.data(), acc[1].data(), cap.data(),
                                     arch[1].data(), success_dev, outSize_dev, archSize_dev, stream);
  HIP(hipStreamSynchronize(stream));
  allSucceeded();
  archSize[1].resize(B);
  HIP(hipMemcpy(archSize[1].data(), archSize_dev, B * 4, hipMemcpyDeviceToHost));
  sameAccumulators();
  for (uint32_t b = 0; b < B; ++b) {
    EXPECT(archSize[0][b] == archSize[1][b]);
    std::vector<uint8_t> x(archSize[0][b]), y(archSize[0][b]);
    HIP(hipMemcpy(x.data(), arch[0][b], x.size(), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(y.data(), arch[1][b], y.size(), hipMemcpyDeviceToHost));
    EXPECT(x == y);
  }

  for (int m = 0; m < 2; ++m) {
    for (uint32_t b = 0; b < B; ++b) {
      HIP(hipFree(acc[m][b]));
      HIP(hipFree(arch[m][b]));
    }
  }
  for (uint32_t k = 0; k < B * S; ++k) {
    HIP(hipFree(comp[k]));
    HIP(hipFree((void*)in[k]));
  }
  HIP(hipFree(compSize_dev));
  HIP(hipFree(outSize_dev));
  HIP(hipFree(archSize_dev));
  HIP(hipFree(success_dev));
  if (failures) {
    printf("reduce_mixed_roundtrip: %d FAILURES\n", failures);
    return 1;
  }
  printf("reduce_mixed_roundtrip: OK\n");
  return 0;
}
