// The norm calls through the C++ mirror (include/dietgpu_amd/GpuAccumulateCodec.h, GpuReduceCompressCodec.h): three bf16
// members of three sources each, the middle source of every member RAW or (sourceKind null) every source an archive.
// floatDecodeReduceNorm must leave fl32(sum * scale) as the host computes it and, per member, the squared norm of those
// words (against a host sum in long double, within n * 2^-52) and a non-finite count of zero; floatReduceCompressNorm the
// same accumulators, byte for byte the archives floatCompressCast writes for them, and the squared norm of the words
// ROUNDED to bfloat16.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuAccumulateCodec.h"
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

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  const std::vector<uint32_t> sizes = {1u, 4097u, 40000u};
  const uint32_t B = (uint32_t)sizes.size(), S = 3;
  const float scale = 1.0f / 3.0f, start = 0.5f;
  std::mt19937 gen(12);
  std::normal_distribution<float> dist(0.0f, 1.0f);
  std::vector<const void*> in(B * S);
  std::vector<void*> comp(B * S);
  std::vector<uint32_t> inSize(B * S), cap(B);
  std::vector<std::vector<float>> wide(B * S);  // the exact float32 value of every bf16 word
  for (uint32_t b = 0; b < B; ++b) {
    for (uint32_t s = 0; s < S; ++s) {
      const uint32_t k = b * S + s;
      std::vector<uint16_t> host(sizes[b]);
      wide[k].resize(sizes[b]);
      for (uint32_t i = 0; i < sizes[b]; ++i) {
        const float f = dist(gen) * (float)(1u << (4u * s));
        uint32_t bits;
        memcpy(&bits, &f, 4);
        host[i] = (uint16_t)(bits >> 16);
        bits &= 0xffff0000u;
        memcpy(&wide[k][i], &bits, 4);
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
  uint32_t *compSize_dev, *outSize_dev, *archSize_dev, *castSize_dev, *nonFinite_dev;
  uint8_t* success_dev;
  double* sumSq_dev;
  HIP(hipMalloc((void**)&nonFinite_dev, B * 4));
  HIP(hipMalloc((void**)&sumSq_dev, B * 8));
  HIP(hipMalloc((void**)&compSize_dev, B * S * 4));
  HIP(hipMalloc((void**)&outSize_dev, B * 4));
  HIP(hipMalloc((void**)&archSize_dev, B * 4));
  HIP(hipMalloc((void**)&castSize_dev, B * 4));
  HIP(hipMalloc((void**)&success_dev, B));
  ANSCodecConfig ans(10, false);
  FloatCodecConfig fc(FloatType::kBFloat16, ans, false, false);
  floatCompress(res, fc, B * S, in.data(), inSize.data(), comp.data(), compSize_dev, stream);
  std::vector<uint32_t> compSize(B * S);
  HIP(hipMemcpyAsync(compSize.data(), compSize_dev, B * S * 4, hipMemcpyDeviceToHost, stream));
  HIP(hipStreamSynchronize(stream));

  std::vector<const void*> plainIn(comp.begin(), comp.end()), mixedIn(plainIn);
  std::vector<uint32_t> plainBytes(compSize), mixedBytes(compSize);
  std::vector<uint8_t> kinds(B * S, 0);
  for (uint32_t b = 0; b < B; ++b) {
    mixedIn[b * S + 1] = in[b * S + 1];
    mixedBytes[b * S + 1] = sizes[b] * 2;
    kinds[b * S + 1] = 1;
  }
  std::vector<float*> acc(B);
  std::vector<void*> arch(B), cast(B);
  for (uint32_t b = 0; b < B; ++b) {
    HIP(hipMalloc((void**)&acc[b], sizes[b] * 4));
    HIP(hipMalloc(&arch[b], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
    HIP(hipMalloc(&cast[b], getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b])));
  }
  auto refill = [&]() {
    for (uint32_t b = 0; b < B; ++b) {
      std::vector<float> v(sizes[b], start);
      HIP(hipMemcpy(acc[b], v.data(), sizes[b] * 4, hipMemcpyHostToDevice));
    }
  };
  // fl32(((start +) x0 + x1 + x2) * scale): every step rounded to float32 (volatile: nothing is fused or kept wider)
  auto expectAccumulators = [&](bool accumulate) {
    for (uint32_t b = 0; b < B; ++b) {
      std::vector<float> got(sizes[b]);
      HIP(hipMemcpy(got.data(), acc[b], sizes[b] * 4, hipMemcpyDeviceToHost));
      uint32_t bad = 0;
      for (uint32_t i = 0; i < sizes[b]; ++i) {
        volatile float sum = accumulate ? start : 0.0f;
        for (uint32_t s = 0; s < S; ++s) {
          if (s == 0 && !accumulate) sum = wide[b * S][i];
          else sum = sum + wide[b * S + s][i];
        }
        volatile float want = sum * scale;
        const float w = want;
        bad += memcmp(&w, &got[i], 4) != 0;
      }
      EXPECT(bad == 0);
    }
  };
  // the squared norm of the words the accumulators hold (rounded: rounded to bfloat16 first, to nearest even), summed on
  // the host in long double; every word of these inputs is finite
  auto expectNorm = [&](bool rounded) {
    std::vector<double> sumSq(B);
    std::vector<uint32_t> nonFinite(B);
    HIP(hipMemcpy(sumSq.data(), sumSq_dev, B * 8, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(nonFinite.data(), nonFinite_dev, B * 4, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < B; ++b) {
      std::vector<float> got(sizes[b]);
      HIP(hipMemcpy(got.data(), acc[b], sizes[b] * 4, hipMemcpyDeviceToHost));
      long double want = 0.0L;
      for (uint32_t i = 0; i < sizes[b]; ++i) {
        uint32_t bits;
        memcpy(&bits, &got[i], 4);
        if (rounded) bits = (bits + 0x7fffu + ((bits >> 16) & 1u)) & 0xffff0000u;
        float w;
        memcpy(&w, &bits, 4);
        want += (long double)w * (long double)w;
      }
      EXPECT(nonFinite[b] == 0);
      EXPECT(std::fabs((double)((long double)sumSq[b] - want)) <= (double)sizes[b] * std::ldexp(1.0, -52) * (double)want);
    }
    const std::vector<double> poison(B, -1.0);
    const std::vector<uint32_t> poisonCount(B, 0xffffffffu);
    HIP(hipMemcpy(sumSq_dev, poison.data(), B * 8, hipMemcpyHostToDevice));
    HIP(hipMemcpy(nonFinite_dev, poisonCount.data(), B * 4, hipMemcpyHostToDevice));
  };
  auto allSucceeded = [&]() {
    std::vector<uint8_t> ok(B);
    std::vector<uint32_t> words(B);
    HIP(hipMemcpy(ok.data(), success_dev, B, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(words.data(), outSize_dev, B * 4, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < B; ++b) EXPECT(ok[b] == 1 && words[b] == sizes[b]);
  };

  for (int mixed = 0; mixed < 2; ++mixed) {
    const void** src = mixed ? mixedIn.data() : plainIn.data();
    const uint32_t* bytes = mixed ? mixedBytes.data() : plainBytes.data();
    const uint8_t* kind = mixed ? kinds.data() : nullptr;  // null: every source is an archive
    for (int accumulate = 0; accumulate < 2; ++accumulate) {
      refill();
      floatDecodeReduceNorm(res, fc, accumulate != 0, B, S, src, bytes, kind, scale, acc.data(), cap.data(), success_dev, outSize_dev, sumSq_dev,
                            nonFinite_dev, stream);
      HIP(hipStreamSynchronize(stream));
      allSucceeded();
      expectAccumulators(accumulate != 0);
      expectNorm(false);

      refill();
      floatReduceCompressNorm(res, fc, accumulate != 0, B, S, src, bytes, kind, scale, acc.data(), cap.data(), arch.data(), success_dev,
                              outSize_dev, archSize_dev, sumSq_dev, nonFinite_dev, stream);
      HIP(hipStreamSynchronize(stream));
      allSucceeded();
      expectAccumulators(accumulate != 0);
      expectNorm(true);
      floatCompressCast(res, fc, B, (const float**)acc.data(), cap.data(), cast.data(), castSize_dev, stream);
      HIP(hipStreamSynchronize(stream));
      std::vector<uint32_t> archSize(B), castSize(B);
      HIP(hipMemcpy(archSize.data(), archSize_dev, B * 4, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(castSize.data(), castSize_dev, B * 4, hipMemcpyDeviceToHost));
      for (uint32_t b = 0; b < B; ++b) {
        EXPECT(archSize[b] == castSize[b]);
        std::vector<uint8_t> x(castSize[b]), y(castSize[b]);
        HIP(hipMemcpy(x.data(), arch[b], x.size(), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(y.data(), cast[b], y.size(), hipMemcpyDeviceToHost));
        EXPECT(x == y);
      }
    }
  }

  for (uint32_t b = 0; b < B; ++b) {
    HIP(hipFree(acc[b]));
    HIP(hipFree(arch[b]));
    HIP(hipFree(cast[b]));
  }
  for (uint32_t k = 0; k < B * S; ++k) {
    HIP(hipFree(comp[k]));
    HIP(hipFree((void*)in[k]));
  }
  HIP(hipFree(compSize_dev));
  HIP(hipFree(outSize_dev));
  HIP(hipFree(archSize_dev));
  HIP(hipFree(castSize_dev));
  HIP(hipFree(success_dev));
  HIP(hipFree(nonFinite_dev));
  HIP(hipFree(sumSq_dev));
  if (failures) {
    printf("reduce_norm_roundtrip: %d FAILURES\n", failures);
    return 1;
  }
  printf("reduce_norm_roundtrip: OK\n");
  return 0;
}
