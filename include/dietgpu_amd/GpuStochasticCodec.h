// Stochastic cast-compress in the style of the dietgpu:: mirror (no reference equivalent): float32 element i is rounded
// STOCHASTICALLY to the config's 16-bit float type in registers -- the neighbour toward zero or the next one away from
// zero, the latter with probability remainder / unit: unbiased, and without the residual of floatCompressFeedback -- and
// compressed into an ordinary float16 / bfloat16 archive, byte for byte what floatCompress writes for the already-rounded
// tensor.  Inline on top of dgpu_float_stochastic_compress of ../dietgpu_amd.h, where the contract is spelled out (the
// rounding rule and the random bits, a pure function of seed, member and word index, are those of
// dgpu_float_decode_update).  `config.floatType` is the type of the ARCHIVE (kFloat16 or kBFloat16); `inSize`: float32
// words.  `seed_dev`: DEVICE memory holding one uint64_t, read by both kernels of the call when they run and never by the
// host; null: the host `seed`.  Member i draws the random bits of member firstMember + i.  The config's useChecksum is
// ignored.  The call takes no temp memory -- its temporaries are the stream's own: there is no StackDeviceMemory parameter.
#pragma once

#include "GpuFloatCodec.h"

namespace dietgpu {

inline void floatCompressStochastic(
    const FloatCompressConfig& config, uint32_t numInBatch, const float** in, const uint32_t* inSize, uint64_t seed,
    const uint64_t* seed_dev, uint32_t firstMember, void** out, uint32_t* outSize_dev, hipStream_t stream) {
  detail::checkRc(dgpu_float_stochastic_compress((uint32_t)config.floatType, config.ansConfig.probBits, numInBatch,
                                                 (const void* const*)in, inSize, seed, seed_dev, firstMember, out, outSize_dev, stream),
                  "floatCompressStochastic");
}

}  // namespace dietgpu
