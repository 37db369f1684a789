// Stochastic cast-compress through the C++ mirror (include/dietgpu_amd/GpuStochasticCodec.h): float32 elements compressed
// with floatCompressStochastic -- a host seed, then a device seed -- for bfloat16 and float16 archives, compared byte for
// byte with archives of words computed on the HOST: every word rounded here by the rule the header states under
// dgpu_float_decode_update (sround_T, r16), uploaded as a 16-bit tensor and compressed with the mirror's plain
// floatCompress.  The inputs sit 4 bytes past a 16-byte boundary and must come back unmodified.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dietgpu_amd/DeviceUtils.h"
#include "dietgpu_amd/GpuStochasticCodec.h"

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

// the contract of dgpu_float_decode_update, on the host
static uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
static uint32_t r16(uint64_t S, uint32_t j, uint32_t k) {
  const uint32_t base = mix32(mix32((uint32_t)S + 0x9E3779B9u) ^ (uint32_t)(S >> 32));
  const uint32_t key = mix32(base + j * 0x85EBCA6Bu);
  const uint32_t bits = mix32(key ^ (k >> 1));
  return (k & 1u) ? bits >> 16 : bits & 0xffffu;
}
static uint16_t sround(uint32_t x, uint32_t r, bool bf16) {
  const uint32_t a = x & 0x7fffffffu, sign = (x >> 16) & 0x8000u;
  if (a > 0x7f800000u) return (uint16_t)(sign | (bf16 ? 0x7fc0u : 0x7e00u));
  if (bf16) return (uint16_t)((x + r) >> 16);
  const uint32_t e = a >> 23, m = (a & 0x7fffffu) | (e ? 0x800000u : 0u);
  const uint32_t shift = 113u - (e > 1u ? e : 1u);
  const uint32_t u = a >= 0x38800000u ? a - 0x38000000u : (shift >= 32u ? 0u : m >> shift);
  const uint32_t h = (u + (r >> 3)) >> 13;
  return (uint16_t)(sign | (h < 0x7c00u ? h : 0x7c00u));
}

int main() {
  DeviceScope scope(getCurrentDevice());
  auto stream = HipStream::makeNonBlocking();
  StackDeviceMemory res(getCurrentDevice(), 64 << 20);
  const std::vector<uint32_t> sizes = {1u, 4097u, 70000u};
  const uint32_t B = (uint32_t)sizes.size(), firstMember = 65534u;
  std::mt19937 gen(17);
  std::normal_distribution<float> dist(0.0f, 1.0f);
  std::vector<std::vector<uint32_t>> host(B);
  std::vector<const float*> in(B);
  std::vector<void*> base(B), got(B), want(B), words(B);
  std::vector<uint32_t> inSize(B), cap(B);
  for (uint32_t b = 0; b < B; ++b) {
    host[b].resize(sizes[b]);
    for (uint32_t i = 0; i < sizes[b]; ++i) {
      const float f = dist(gen) * (float)(1 << (i % 12));
      memcpy(&host[b][i], &f, 4);
      if (i % 1000 == 7) host[b][i] = gen();  // any 32 bits: NaNs, infinities, denormals
    }
    HIP(hipMalloc(&base[b], sizes[b] * 4 + 16));
    in[b] = (const float*)((uint8_t*)base[b] + 4);
    HIP(hipMemcpyAsync((void*)in[b], host[b].data(), sizes[b] * 4, hipMemcpyHostToDevice, stream));
    inSize[b] = sizes[b];
    cap[b] = getMaxFloatCompressedSize(FloatType::kBFloat16, sizes[b]);
    HIP(hipMalloc(&got[b], cap[b]));
    HIP(hipMalloc(&want[b], cap[b]));
    HIP(hipMalloc(&words[b], sizes[b] * 2));
  }
  uint32_t *gotSize_dev, *wantSize_dev;
  uint64_t* seed_dev;
  HIP(hipMalloc((void**)&gotSize_dev, B * 4));
  HIP(hipMalloc((void**)&wantSize_dev, B * 4));
  HIP(hipMalloc((void**)&seed_dev, 8));
  const uint64_t seed = 0xfedcba9876543210ull;
  HIP(hipMemcpyAsync(seed_dev, &seed, 8, hipMemcpyHostToDevice, stream));
  HIP(hipStreamSynchronize(stream));

  for (const FloatType ft : {FloatType::kBFloat16, FloatType::kFloat16}) {
    ANSCodecConfig ans(10, false);
    FloatCodecConfig fc(ft, ans, false, false);
    // pass 0: a host seed; pass 1: the device seed (the host value beside it is not looked at)
    for (int pass = 0; pass < 2; ++pass) {
      const uint64_t S = pass ? seed : 12345u;
      for (uint32_t b = 0; b < B; ++b) {
        std::vector<uint16_t> q(sizes[b]);
        for (uint32_t k = 0; k < sizes[b]; ++k) q[k] = sround(host[b][k], r16(S, firstMember + b, k), ft == FloatType::kBFloat16);
        HIP(hipMemcpyAsync(words[b], q.data(), sizes[b] * 2, hipMemcpyHostToDevice, stream));
        HIP(hipMemsetAsync(got[b], 0, cap[b], stream));
        HIP(hipMemsetAsync(want[b], 0, cap[b], stream));
        HIP(hipStreamSynchronize(stream));
      }
      std::vector<const void*> wordsIn(words.begin(), words.end());
      floatCompress(res, fc, B, wordsIn.data(), inSize.data(), want.data(), wantSize_dev, stream);
      floatCompressStochastic(fc, B, in.data(), inSize.data(), pass ? 99u : S, pass ? seed_dev : nullptr, firstMember, got.data(), gotSize_dev,
                              stream);
      std::vector<uint32_t> gotSize(B), wantSize(B);
      HIP(hipMemcpyAsync(gotSize.data(), gotSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
      HIP(hipMemcpyAsync(wantSize.data(), wantSize_dev, B * 4, hipMemcpyDeviceToHost, stream));
      HIP(hipStreamSynchronize(stream));
      for (uint32_t b = 0; b < B; ++b) {
        EXPECT(gotSize[b] == wantSize[b] && gotSize[b] != 0 && gotSize[b] <= cap[b]);
        std::vector<uint8_t> g(wantSize[b]), w(wantSize[b]);
        std::vector<uint32_t> back(sizes[b]);
        HIP(hipMemcpyAsync(g.data(), got[b], g.size(), hipMemcpyDeviceToHost, stream));
        HIP(hipMemcpyAsync(w.data(), want[b], w.size(), hipMemcpyDeviceToHost, stream));
        HIP(hipMemcpyAsync(back.data(), in[b], sizes[b] * 4, hipMemcpyDeviceToHost, stream));
        HIP(hipStreamSynchronize(stream));
        EXPECT(g == w);
        EXPECT(back == host[b]);  // the input is not modified
      }
    }
  }
  for (uint32_t b = 0; b < B; ++b) {
    HIP(hipFree(base[b]));
    HIP(hipFree(got[b]));
    HIP(hipFree(want[b]));
    HIP(hipFree(words[b]));
  }
  HIP(hipFree(gotSize_dev));
  HIP(hipFree(wantSize_dev));
  HIP(hipFree(seed_dev));
  if (failures) {
    printf("stochastic_api: %d FAILURES\n", failures);
    return 1;
  }
  printf("stochastic_api: OK\n");
  return 0;
}
