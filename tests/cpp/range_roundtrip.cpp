// Ranged decode through the C++ mirror (include/dietgpu_amd/GpuRangeCodec.h): archives made with ansEncodeBatchPointer /
// floatCompress, block ranges of them decoded with ansDecodeBatchPointerRange / floatDecompressRange and compared with
// the input, guard words around every output.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuRangeCodec.h"

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

struct Range {
  uint32_t first, count;
};

// T = uint8_t (raw bytes) or uint16_t (bfloat16 bit patterns)
template <typename T>
static void rangesOf(StackDeviceMemory& res, hipStream_t stream, bool asFloat) {
  const std::vector<uint32_t> sizes = {4096u * 5u + 1234u, 4096u * 17u, 4096u * 3u};
  const std::vector<Range> ranges = {{1, 4}, {15, 2}, {3, kToEndOfElement}};  // odd start; across a tile edge; empty at the end
  const uint32_t B = (uint32_t)sizes.size(), guard = 64 / sizeof(T);
  std::mt19937 gen(5);
  std::normal_distribution<float> dist(0.0f, 1.0f);
  std::vector<std::vector<T>> host(B);
  std::vector<const void*> in(B);
  std::vector<void*> comp(B), out(B);
  std::vector<uint32_t> inSize(B), compCap(B), first(B), count(B), cap(B), want(B);
  for (uint32_t b = 0; b < B; ++b) {
    host[b].resize(sizes[b]);
    for (auto& v : host[b]) {
      float f = dist(gen);
      uint32_t bits;
      memcpy(&bits, &f, 4);
      v = asFloat ? (T)(bits >> 16) : (T)(bits >> 20);
    }
    T* d = nullptr;
    HIP(hipMalloc((void**)&d, sizes[b] * sizeof(T)));
    HIP(hipMemcpyAsync(d, host[b].data(), sizes[b] * sizeof(T), hipMemcpyHostToDevice, stream));
    in[b] = d;
    inSize[b] = sizes[b];
    compCap[b] = asFloat ? getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b]) : getMaxCompressedSize(sizes[b]);
    HIP(hipMalloc(&comp[b], compCap[b]));
    first[b] = ranges[b].first;
    count[b] = ranges[b].count;
    const uint64_t lo = (uint64_t)first[b] * kRangeBlockWords;
    const uint64_t hi = std::min<uint64_t>(sizes[b], ((uint64_t)first[b] + count[b]) * kRangeBlockWords);
    want[b] = (uint32_t)(hi - lo);
    cap[b] = want[b];
    T* o = nullptr;
    HIP(hipMalloc((void**)&o, (want[b] + 2 * guard) * sizeof(T)));
    HIP(hipMemsetAsync(o, 0xcd, (want[b] + 2 * guard) * sizeof(T), stream));
    out[b] = o + guard;
  }
  uint32_t* compSize_dev;
  uint32_t* outSize_dev;
  uint8_t* success_dev;
  HIP(hipMalloc((void**)&compSize_dev, B * 4));
  HIP(hipMalloc((void**)&outSize_dev, B * 4));
  HIP(hipMalloc((void**)&success_dev, B));
  ANSCodecConfig ans(10, false);
  FloatCodecConfig fc(FloatType::kBFloat16, ans, false, true);  // (a float checksum in the archive: ignored by ranges)
  if (asFloat) floatCompress(res, fc, B, in.data(), inSize.data(), comp.data(), compSize_dev, stream);
  else ansEncodeBatchPointer(res, ans, B, in.data(), inSize.data(), nullptr, comp.data(), compSize_dev, stream);
  std::vector<uint32_t> compSize(B);
  HIP(hipMemcpyAsync(compSize.data(), compSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
  HIP(hipStreamSynchronize(stream));
  std::vector<const void*> compIn(comp.begin(), comp.end());
  if (asFloat) {
    floatDecompressRange(res, fc, B, compIn.data(), compSize.data(), first.data(), count.data(), out.data(), cap.data(),
                         success_dev, outSize_dev, stream);
  } else {
    ansDecodeBatchPointerRange(res, ans, B, compIn.data(), compSize.data(), first.data(), count.data(), out.data(),
                               cap.data(), success_dev, outSize_dev, stream);
  }
  std::vector<uint32_t> outSize(B);
  std::vector<uint8_t> success(B);
  HIP(hipMemcpyAsync(outSize.data(), outSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
  HIP(hipMemcpyAsync(success.data(), success_dev, B, hipMemcpyDeviceToHost, stream));
  for (uint32_t b = 0; b < B; ++b) {
    std::vector<T> got(want[b] + 2 * guard);
    HIP(hipMemcpyAsync(got.data(), (T*)out[b] - guard, got.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP(hipStreamSynchronize(stream));
    EXPECT(success[b] == 1);
    EXPECT(outSize[b] == want[b]);
    EXPECT(memcmp(got.data() + guard, host[b].data() + (size_t)first[b] * kRangeBlockWords, want[b] * sizeof(T)) == 0);
    for (uint32_t g = 0; g < guard; ++g) {
      EXPECT(got[g] == (T)0xcdcdcdcdu);
      EXPECT(got[guard + want[b] + g] == (T)0xcdcdcdcdu);
    }
    HIP(hipFree((T*)out[b] - guard));
    HIP(hipFree(comp[b]));
    HIP(hipFree((void*)in[b]));
  }
  HIP(hipFree(compSize_dev));
  HIP(hipFree(outSize_dev));
  HIP(hipFree(success_dev));
}

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  rangesOf<uint8_t>(res, stream, false);
  rangesOf<uint16_t>(res, stream, true);
  HIP(hipStreamSynchronize(stream));
  if (failures) {
    printf("range_roundtrip: %d FAILURES\n", failures);
    return 1;
  }
  printf("range_roundtrip: OK\n");
  return 0;
}
