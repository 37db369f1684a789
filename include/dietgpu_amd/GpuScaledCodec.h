// Scaled decompress in the style of the dietgpu:: mirror (no reference equivalent): float archive i is decoded into
// out[i] with every word multiplied by a float32 factor before it is stored -- one IEEE float32 multiply and one rounding
// to the archive's type -- so the clip coefficient of a compressed all-reduce is applied by the decode of its final
// all-gather.  Inline on top of dgpu_float_decode_scaled of ../dietgpu_amd.h, where the contract is spelled out.
// `inBytes`: the bytes available at in[i]; `outCapacity`: float words.  `scale_dev`: DEVICE memory holding 1 float
// (scaleStride 0: one factor for the call) or numInBatch floats (scaleStride 1), read when the kernel runs and never by
// the host -- it may hold any value; null: the host float `scale`, which must be finite and not zero.  The config's
// useChecksum is ignored: a checksum covers the stored words of the original tensor, which this call does not leave.
// Uses no temp memory.
#pragma once

#include "GpuFloatCodec.h"

namespace dietgpu {

inline void floatDecompressScaled(
    StackDeviceMemory& res, const FloatDecompressConfig& config, uint32_t numInBatch, const void** in, const uint32_t* inBytes,
    void** out, const uint32_t* outCapacity, float scale, const float* scale_dev, uint32_t scaleStride, uint8_t* outSuccess_dev,
    uint32_t* outSize_dev, hipStream_t stream) {
  (void)res;
  size_t used = 0;
  detail::checkRc(dgpu_float_decode_scaled(nullptr, 0, &used, (uint32_t)config.floatType, config.ansConfig.probBits, numInBatch,
                                               in, inBytes, (void* const*)out, outCapacity, scale, scale_dev, scaleStride,
                                               outSuccess_dev, outSize_dev, stream),
                  "floatDecompressScaled");
}

}  // namespace dietgpu
