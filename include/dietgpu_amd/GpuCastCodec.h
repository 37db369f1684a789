// Cast-compress in the style of the dietgpu:: mirror (no reference equivalent): float32 element i is rounded to the
// config's 16-bit float type in registers and compressed into an ordinary float16 / bfloat16 archive, byte for byte what
// floatCompress writes for the already-rounded tensor.  Inline on top of dgpu_float_cast_compress of ../dietgpu_amd.h,
// where the rounding and the contract are spelled out.  `config.floatType` is the type of the ARCHIVE (kFloat16 or
// kBFloat16); `inSize`: float32 words.  The config's useChecksum is ignored: a checksum covers the 16-bit words, which
// never reach memory here.
#pragma once

#include "GpuFloatCodec.h"

namespace dietgpu {

inline void floatCompressCast(
    StackDeviceMemory& res, const FloatCompressConfig& config, uint32_t numInBatch, const float** in, const uint32_t* inSize,
    void** out, uint32_t* outSize_dev, hipStream_t stream) {
  uint32_t maxSize = 0;
  for (uint32_t i = 0; i < numInBatch; ++i) maxSize = std::max(maxSize, inSize[i]);
  detail::TempRegion t(res, stream, dgpu_float_compress_temp_bytes((uint32_t)config.floatType, numInBatch, maxSize));
  detail::checkRc(dgpu_float_cast_compress(t.ptr, t.bytes, &t.used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                           numInBatch, (const void* const*)in, inSize, out, outSize_dev, stream),
                  "floatCompressCast");
}

}  // namespace dietgpu
