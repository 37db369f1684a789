// Feedback cast-compress in the style of the dietgpu:: mirror (no reference equivalent): float32 element i plus its
// float32 residual is rounded to the config's 16-bit float type in registers and compressed into an ordinary float16 /
// bfloat16 archive, and the rounding error is stored as the next step's residual.  Inline on top of
// dgpu_float_feedback_compress of ../dietgpu_amd.h, where the four steps and the contract are spelled out.
// `config.floatType` is the type of the ARCHIVE (kFloat16 or kBFloat16); `inSize`: float32 words; `residualIn`: the
// array may be null (no residual yet), and residualOut[i] may equal residualIn[i] (in place: the intended use).  The
// config's useChecksum is ignored, as by floatCompressCast.
#pragma once

#include "GpuFloatCodec.h"

namespace dietgpu {

inline void floatCompressFeedback(
    StackDeviceMemory& res, const FloatCompressConfig& config, uint32_t numInBatch, const float** in, const uint32_t* inSize,
    const float** residualIn, float** residualOut, void** out, uint32_t* outSize_dev, hipStream_t stream) {
  uint32_t maxSize = 0;
  for (uint32_t i = 0; i < numInBatch; ++i) maxSize = std::max(maxSize, inSize[i]);
  detail::TempRegion t(res, stream, dgpu_float_compress_temp_bytes((uint32_t)config.floatType, numInBatch, maxSize));
  detail::checkRc(dgpu_float_feedback_compress(t.ptr, t.bytes, &t.used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                               numInBatch, (const void* const*)in, inSize, (const void* const*)residualIn,
                                               (void* const*)residualOut, out, outSize_dev, stream),
                  "floatCompressFeedback");
}

}  // namespace dietgpu
