// Reduce-compress through the C++ mirror (include/dietgpu_amd/GpuReduceCompressCodec.h): three bf16 members of three
// sources each, compressed with floatCompress; floatDecompressReduceCompress with accumulate = false and then true.  The
// accumulators are compared bit for bit with the left-to-right float32 sum made on the host (guard words around every
// one), the archives byte for byte with what floatCompressCast writes for the accumulators afterwards, and they decode
// (floatDecompress) to the sums rounded to bfloat16 on the host.  Then one source truncated: its member fails and keeps
// its bits, and its archive still decodes -- to the rounding of what the accumulator holds.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuCastCodec.h"
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
// float32 bits -> bfloat16, round to nearest even, NaN to the canonical quiet NaN with its sign (dietgpu_amd.h)
static uint16_t roundBf16(uint32_t x) {
  if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)(((x >> 16) & 0x8000u) | 0x7fc0u);
  return (uint16_t)((x + 0x7fffu + ((x >> 16) & 1u)) >> 16);
}

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  const std::vector<uint32_t> sizes = {1u, 4097u, 40000u};
  const uint32_t B = (uint32_t)sizes.size(), S = 3, guard = 64;
  const uint32_t kSentinel = 0xcdcdcdcdu;
  std::mt19937 gen(12);
  std::normal_distribution<float> dist(0.0f, 1.0f);
  // member-major: source s of member b at b * S + s
  std::vector<std::vector<uint16_t>> host(B * S);
  std::vector<const void*> in(B * S);
  std::vector<void*> comp(B * S), archive(B), archive2(B), decoded(B);
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
    HIP(hipMalloc(&archive[b], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    HIP(hipMalloc(&archive2[b], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    HIP(hipMalloc(&decoded[b], sizes[b] * 2));
  }
  uint32_t *compSize_dev, *outSize_dev, *archiveSize_dev, *archiveSize2_dev, *decodedSize_dev;
  uint8_t *success_dev, *decodedOk_dev;
  HIP(hipMalloc((void**)&compSize_dev, B * S * 4));
  HIP(hipMalloc((void**)&outSize_dev, B * 4));
  HIP(hipMalloc((void**)&archiveSize_dev, B * 4));
  HIP(hipMalloc((void**)&archiveSize2_dev, B * 4));
  HIP(hipMalloc((void**)&decodedSize_dev, B * 4));
  HIP(hipMalloc((void**)&success_dev, B));
  HIP(hipMalloc((void**)&decodedOk_dev, B));
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
    floatDecompressReduceCompress(res, fc, pass >= 1, B, S, compIn.data(), offered.data(), acc.data(), cap.data(), archive.data(),
                                  success_dev, outSize_dev, archiveSize_dev, stream);
    // the two-call path's second half, on the accumulators the one call left
    std::vector<const float*> accIn(acc.begin(), acc.end());
    floatCompressCast(res, fc, B, accIn.data(), cap.data(), archive2.data(), archiveSize2_dev, stream);
    std::vector<const void*> archiveIn(archive.begin(), archive.end());
    floatDecompress(res, fc, B, archiveIn.data(), decoded.data(), cap.data(), decodedOk_dev, decodedSize_dev, stream);
    std::vector<uint32_t> outSize(B), archiveSize(B), archiveSize2(B), decodedSize(B);
    std::vector<uint8_t> success(B), decodedOk(B);
    HIP(hipMemcpyAsync(outSize.data(), outSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(archiveSize.data(), archiveSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(archiveSize2.data(), archiveSize2_dev, B * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(decodedSize.data(), decodedSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(success.data(), success_dev, B, hipMemcpyDeviceToHost, stream));
    HIP(hipMemcpyAsync(decodedOk.data(), decodedOk_dev, B, hipMemcpyDeviceToHost, stream));
    HIP(hipStreamSynchronize(stream));
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
      // the archive: inside the bound, decodable to the rounded accumulator; for a successful member the bytes of
      // cast-compress
      EXPECT(archiveSize[b] <= getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b]));
      EXPECT(decodedOk[b] == 1 && decodedSize[b] == sizes[b]);
      std::vector<uint16_t> words(sizes[b]);
      HIP(hipMemcpy(words.data(), decoded[b], sizes[b] * 2, hipMemcpyDeviceToHost));
      uint32_t badWords = 0;
      for (uint32_t i = 0; i < sizes[b]; ++i) badWords += words[i] != roundBf16(want[b][i]);
      EXPECT(badWords == 0);
      if (!fails) {
        EXPECT(archiveSize[b] == archiveSize2[b]);
        std::vector<uint8_t> one(archiveSize[b]), two(archiveSize[b]);
        HIP(hipMemcpy(one.data(), archive[b], one.size(), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(two.data(), archive2[b], two.size(), hipMemcpyDeviceToHost));
        EXPECT(one == two);
      }
    }
  }
  for (uint32_t b = 0; b < B; ++b) {
    HIP(hipFree(acc[b] - guard));
    HIP(hipFree(archive[b]));
    HIP(hipFree(archive2[b]));
    HIP(hipFree(decoded[b]));
  }
  for (uint32_t k = 0; k < B * S; ++k) {
    HIP(hipFree(comp[k]));
    HIP(hipFree((void*)in[k]));
  }
  HIP(hipFree(compSize_dev));
  HIP(hipFree(outSize_dev));
  HIP(hipFree(archiveSize_dev));
  HIP(hipFree(archiveSize2_dev));
  HIP(hipFree(decodedSize_dev));
  HIP(hipFree(success_dev));
  HIP(hipFree(decodedOk_dev));
  if (failures) {
    printf("reduce_compress_roundtrip: %d FAILURES\n", failures);
    return 1;
  }
  printf("reduce_compress_roundtrip: OK\n");
  return 0;
}
