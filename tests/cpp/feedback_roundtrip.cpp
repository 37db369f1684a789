// Feedback cast-compress through the C++ mirror (include/dietgpu_amd/GpuFeedbackCodec.h): two in-place steps of a batch
// of three float32 elements into bfloat16 archives with floatCompressFeedback -- the first without a residual, the second
// with the one the first left -- each decoded with floatDecompress.  Words and residuals equal a host loop of the four
// steps of the contract (add, round to nearest even on the bits, exact difference, zero where the word is not finite),
// and the inputs are unchanged.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuFeedbackCodec.h"

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
static float asFloat(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
static uint32_t asBits(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}
// one word of the contract: x and the residual (have: there is one) -> the 16-bit word; the residual is updated
static uint16_t feedbackStep(uint32_t x, uint32_t& e, bool have) {
  volatile float sum = asFloat(x) + asFloat(e);  // (one float32 add, kept out of any wider evaluation)
  const uint32_t v = have ? asBits(sum) : x;
  const uint16_t q = roundToBf16(v);
  const uint32_t w = (uint32_t)q << 16;
  volatile float diff = asFloat(v) - asFloat(w);
  e = (w & 0x7f800000u) == 0x7f800000u ? 0u : asBits(diff);
  return q;
}

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  const std::vector<uint32_t> sizes = {3u, 4097u, 40000u};
  const uint32_t B = (uint32_t)sizes.size();
  std::mt19937 gen(13);
  std::normal_distribution<float> dist(0.0f, 1.0f);
  std::vector<std::vector<uint32_t>> host(B), wantRes(B);
  std::vector<const float*> in(B);
  std::vector<float*> residual(B);
  std::vector<void*> comp(B), out(B);
  std::vector<uint32_t> inSize(B);
  for (uint32_t b = 0; b < B; ++b) {
    host[b].resize(sizes[b]);
    wantRes[b].assign(sizes[b], 0u);
    for (uint32_t i = 0; i < sizes[b]; ++i) {
      host[b][i] = asBits(dist(gen));
      if (i % 97 == 5) host[b][i] = 0x3f808000u;   // a tie: half a unit of the last place is left over
      if (i % 101 == 7) host[b][i] = 0x7f7f8000u;  // overflows to infinity: the residual is zero
      if (i % 103 == 9) host[b][i] = 0x80000000u;  // -0 keeps its sign in the first step
      if (i % 107 == 11) host[b][i] = 0x7f800001u; // a NaN
    }
    float* d = nullptr;
    HIP(hipMalloc((void**)&d, sizes[b] * 4));
    HIP(hipMemcpyAsync(d, host[b].data(), sizes[b] * 4, hipMemcpyHostToDevice, stream));
    in[b] = d;
    inSize[b] = sizes[b];
    HIP(hipMalloc((void**)&residual[b], sizes[b] * 4));
    HIP(hipMemsetAsync(residual[b], 0xff, sizes[b] * 4, stream));  // NaNs: the first step must not read them
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
  std::vector<const float*> residualIn(residual.begin(), residual.end());
  for (int step = 0; step < 2; ++step) {
    floatCompressFeedback(res, fc, B, in.data(), inSize.data(), step == 0 ? nullptr : residualIn.data(), residual.data(), comp.data(),
                          compSize_dev, stream);
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
      std::vector<uint32_t> src(sizes[b]), gotRes(sizes[b]);
      HIP(hipMemcpyAsync(got.data(), out[b], sizes[b] * 2, hipMemcpyDeviceToHost, stream));
      HIP(hipMemcpyAsync(src.data(), in[b], sizes[b] * 4, hipMemcpyDeviceToHost, stream));
      HIP(hipMemcpyAsync(gotRes.data(), residual[b], sizes[b] * 4, hipMemcpyDeviceToHost, stream));
      HIP(hipStreamSynchronize(stream));
      EXPECT(success[b] == 1);
      EXPECT(outSize[b] == sizes[b]);
      EXPECT(compSize[b] > 16 && compSize[b] <= getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b]));
      uint32_t bad = 0, badRes = 0, changed = 0;
      for (uint32_t i = 0; i < sizes[b]; ++i) {
        const uint16_t q = feedbackStep(host[b][i], wantRes[b][i], step != 0);
        bad += got[i] != q;
        badRes += gotRes[i] != wantRes[b][i];
        changed += src[i] != host[b][i];
      }
      EXPECT(bad == 0);
      EXPECT(badRes == 0);
      EXPECT(changed == 0);
    }
  }
  for (uint32_t b = 0; b < B; ++b) {
    HIP(hipFree(out[b]));
    HIP(hipFree(comp[b]));
    HIP(hipFree(residual[b]));
    HIP(hipFree((void*)in[b]));
  }
  HIP(hipFree(compSize_dev));
  HIP(hipFree(outSize_dev));
  HIP(hipFree(success_dev));
  if (failures) {
    printf("feedback_roundtrip: %d FAILURES\n", failures);
    return 1;
  }
  printf("feedback_roundtrip: OK\n");
  return 0;
}
