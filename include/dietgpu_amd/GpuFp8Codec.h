// FP8 archives in the style of the dietgpu:: mirror (no reference equivalent): the FP8 wire of a compressed exchange of
// float32 gradients.  fp8CompressCast writes, for every tensor, the ordinary raw-byte ANS archive of its words multiplied
// by a factor and rounded to an OCP FP8 type (e4m3fn or e5m2; round to nearest even, no saturation) -- byte for byte what
// ansEncodeBatchPointer writes for the FP8 bytes, without a checksum -- and fp8DecompressAccumulate widens every decoded
// byte to float32, multiplies it by a factor and stores it to or adds it into a float32 accumulator; a member that
// fails keeps every bit of its accumulator.  Both convert in the codec's own kernels: the FP8 tensor never exists in
// memory.  Inline on top of dgpu_fp8_cast_compress / dgpu_fp8_decode_accumulate of ../dietgpu_amd.h, where the contract
// is spelled out.  `inSize`, `accWords`: float32 words; `inBytes`: bytes.  scale_dev: device memory read by the kernels
// (one factor, or one per member with scalePerMember), or null for the host float `scale` (finite, not zero).  The
// config's useChecksum is ignored.  Neither call takes temp memory: there is no StackDeviceMemory parameter.
#pragma once

#include "GpuANSCodec.h"

namespace dietgpu {

enum class Fp8Type : uint32_t { kE4M3FN = DGPU_FP8_E4M3FN, kE5M2 = DGPU_FP8_E5M2 };

inline void fp8CompressCast(
    const ANSCodecConfig& config, Fp8Type type, uint32_t numInBatch, const void** in, const uint32_t* inSize, float scale,
    const float* scale_dev, bool scalePerMember, void** out, uint32_t* outSize_dev, hipStream_t stream) {
  detail::checkRc(dgpu_fp8_cast_compress((uint32_t)type, config.probBits, numInBatch, in, inSize, scale, scale_dev, scalePerMember ? 1u : 0u, out,
                                         outSize_dev, stream),
                  "fp8CompressCast");
}

inline void fp8DecompressAccumulate(
    const ANSCodecConfig& config, Fp8Type type, bool accumulate, uint32_t numInBatch, const void** in, const uint32_t* inBytes,
    float scale, const float* scale_dev, bool scalePerMember, void** acc, const uint32_t* accWords, uint8_t* outSuccess_dev,
    uint32_t* outSize_dev, hipStream_t stream) {
  detail::checkRc(dgpu_fp8_decode_accumulate((uint32_t)type, config.probBits, accumulate ? 1 : 0, numInBatch, in, inBytes, scale, scale_dev,
                                             scalePerMember ? 1u : 0u, acc, accWords, outSuccess_dev, outSize_dev, stream),
                  "fp8DecompressAccumulate");
}

}  // namespace dietgpu
