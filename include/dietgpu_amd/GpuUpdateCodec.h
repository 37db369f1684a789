// Decode-update in the style of the dietgpu:: mirror (no reference equivalent): 16-bit float archive i is decoded,
// multiplied by a float32 factor, added to (accumulate) or stored over the 16-bit tensor out[i] of the archive's type, and
// rounded STOCHASTICALLY back to that type -- out[i][k] = sround_T([widen(out[i][k]) +] fl32(widen(word) * s)), one IEEE
// multiply and one IEEE add, never fused -- so the final all-gather of a compressed all-reduce updates bfloat16 / float16
// parameters that have no float32 master copy.  Inline on top of dgpu_float_decode_update of ../dietgpu_amd.h, where the
// contract (the rounding rule and the random bits, a pure function of seed, member and word index) is spelled out.
// `inBytes`: the bytes available at in[i]; `outCapacity`: words.  `scale_dev`: DEVICE memory holding 1 float (scaleStride
// 0) or numInBatch floats (scaleStride 1), read when the kernel runs and never by the host; null: the host float `scale`,
// which must be finite and not zero.  `seed_dev`: DEVICE memory holding one uint64_t, read when the kernel runs; null: the
// host `seed`.  Member i draws the random bits of member firstMember + i.  config.floatType must be kFloat16 or kBFloat16;
// the config's useChecksum is ignored.  No temp memory is used: there is no StackDeviceMemory parameter.
#pragma once

#include "GpuFloatCodec.h"

namespace dietgpu {

inline void floatDecompressUpdate(
    const FloatDecompressConfig& config, bool accumulate, uint32_t numInBatch, const void** in, const uint32_t* inBytes, void** out,
    const uint32_t* outCapacity, float scale, const float* scale_dev, uint32_t scaleStride, uint64_t seed, const uint64_t* seed_dev,
    uint32_t firstMember, uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  detail::checkRc(dgpu_float_decode_update((uint32_t)config.floatType, config.ansConfig.probBits, accumulate ? 1 : 0, numInBatch, in,
                                           inBytes, (void* const*)out, outCapacity, scale, scale_dev, scaleStride, seed, seed_dev,
                                           firstMember, outSuccess_dev, outSize_dev, stream),
                  "floatDecompressUpdate");
}

}  // namespace dietgpu
