// Ranged decode in the style of the dietgpu:: mirror (no reference equivalent): blocks
// [firstBlock[i], firstBlock[i] + numBlocks[i]) of archive i -- 4096 words each -- into out[i], which holds the range,
// without reading the rest of the archive.  Inline on top of dgpu_ans_decode_batch_pointer_range /
// dgpu_float_decompress_range of ../dietgpu_amd.h, where the contract is spelled out.  `inBytes`: the bytes available
// at in[i].  numBlocks[i] == kToEndOfElement: to the end.  The configs' useChecksum is ignored: a checksum covers the
// whole element and cannot be verified from a part of it.
#pragma once

#include "GpuFloatCodec.h"

namespace dietgpu {

constexpr uint32_t kRangeBlockWords = 4096;
constexpr uint32_t kToEndOfElement = 0xffffffffu;

inline void ansDecodeBatchPointerRange(
    StackDeviceMemory& res, const ANSCodecConfig& config, uint32_t numInBatch, const void** in, const uint32_t* inBytes,
    const uint32_t* firstBlock, const uint32_t* numBlocks, void** out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  uint32_t maxCap = 0;
  for (uint32_t i = 0; i < numInBatch; ++i) maxCap = std::max(maxCap, outCapacity[i]);
  detail::TempRegion t(res, stream, dgpu_ans_decode_temp_bytes(numInBatch, maxCap, config.probBits));
  detail::checkRc(dgpu_ans_decode_batch_pointer_range(t.ptr, t.bytes, &t.used, config.probBits, numInBatch, in, inBytes,
                                                      firstBlock, numBlocks, out, outCapacity, outSuccess_dev,
                                                      outSize_dev, stream),
                  "ansDecodeBatchPointerRange");
}

inline void floatDecompressRange(
    StackDeviceMemory& res, const FloatDecompressConfig& config, uint32_t numInBatch, const void** in,
    const uint32_t* inBytes, const uint32_t* firstBlock, const uint32_t* numBlocks, void** out,
    const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  uint32_t maxCap = 0;
  for (uint32_t i = 0; i < numInBatch; ++i) maxCap = std::max(maxCap, outCapacity[i]);
  detail::TempRegion t(res, stream, dgpu_float_decompress_temp_bytes((uint32_t)config.floatType, numInBatch, maxCap,
                                                                     config.ansConfig.probBits));
  detail::checkRc(dgpu_float_decompress_range(t.ptr, t.bytes, &t.used, (uint32_t)config.floatType,
                                              config.ansConfig.probBits, numInBatch, in, inBytes, firstBlock, numBlocks,
                                              out, outCapacity, outSuccess_dev, outSize_dev, stream),
                  "floatDecompressRange");
}

}  // namespace dietgpu
