// Rolling-table compress in the style of the dietgpu:: mirror (no reference equivalent): floatCompress / floatCompressCast
// for tensors that come back step after step.  The table of a call is made from the exponent counts the LAST call left
// (countsIn_dev: no histogram pass reads the input) and the encoder leaves this call's counts for the NEXT one
// (countsOut_dev); both are device arrays [numInBatch][256], either may be null and they may be the same buffer.  Inline
// on top of dgpu_float_rolling_compress of ../dietgpu_amd.h, where the contract is spelled out: any counts give a
// lossless archive every decoder reads, a reported size above getMaxFloatCompressedSize means an incomplete archive
// (compress again with countsIn_dev = nullptr).  `config.floatType` is the type of the ARCHIVE (kFloat16 or kBFloat16);
// `sourceFloat32`: in[i] holds float32 words, rounded as by floatCompressCast.  The config's useChecksum is ignored.
#pragma once

#include "GpuFloatCodec.h"

namespace dietgpu {

inline void floatCompressRolling(
    StackDeviceMemory& res, const FloatCompressConfig& config, bool sourceFloat32, uint32_t numInBatch, const void** in,
    const uint32_t* inSize, const uint32_t* countsIn_dev, uint32_t* countsOut_dev, void** out, uint32_t* outSize_dev,
    hipStream_t stream) {
  uint32_t maxSize = 0;
  for (uint32_t i = 0; i < numInBatch; ++i) maxSize = std::max(maxSize, inSize[i]);
  detail::TempRegion t(res, stream, dgpu_float_compress_temp_bytes((uint32_t)config.floatType, numInBatch, maxSize));
  detail::checkRc(dgpu_float_rolling_compress(t.ptr, t.bytes, &t.used, (uint32_t)config.floatType, sourceFloat32 ? 1u : 0u,
                                              config.ansConfig.probBits, numInBatch, (const void* const*)in, inSize, countsIn_dev,
                                              countsOut_dev, out, outSize_dev, stream),
                  "floatCompressRolling");
}

}  // namespace dietgpu
