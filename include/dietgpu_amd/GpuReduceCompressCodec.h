// Reduce-compress in the style of the dietgpu:: mirror (no reference equivalent): floatDecompressReduce into the float32
// accumulators and floatCompressCast of those accumulators back to the sources' 16-bit type in ONE call, which counts
// the exponents of the rounded sums while it stores them instead of reading the accumulators again for a histogram --
// the middle of a compressed all-reduce.  Inline on top of dgpu_float_reduce_compress of ../dietgpu_amd.h, where the
// contract is spelled out.  `config.floatType` is the type of the sources AND of the archives (kFloat16 or kBFloat16);
// sources are member-major (source s of member i is in[i * numSources + s], inBytes of the same shape) and must state
// exactly outCapacity[i] words; acc, outCapacity (float words), outArchive, outSuccess_dev, outSize_dev (words) and
// outArchiveSize_dev (bytes) have numInBatch entries; outArchive[i] has room for getMaxFloatCompressedSize of
// outCapacity[i].  A member with outSuccess_dev[i] = 0 keeps its accumulator; its archive holds whatever the accumulator
// held.  The config's useChecksum is ignored, as in the two halves.
#pragma once

#include "GpuFloatCodec.h"

namespace dietgpu {

inline void floatDecompressReduceCompress(
    StackDeviceMemory& res, const FloatDecompressConfig& config, bool accumulate, uint32_t numInBatch, uint32_t numSources,
    const void** in, const uint32_t* inBytes, float** acc, const uint32_t* outCapacity, void** outArchive,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, uint32_t* outArchiveSize_dev, hipStream_t stream) {
  detail::ReduceTemp t(res, stream, outCapacity, numInBatch,
                       [&](uint32_t maxWords) { return dgpu_float_reduce_compress_temp_bytes((uint32_t)config.floatType, numInBatch, maxWords); });
  detail::checkRc(dgpu_float_reduce_compress(t.ptr, t.bytes, &t.used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                             accumulate ? 1 : 0, numInBatch, numSources, in, inBytes, (void* const*)acc,
                                             outCapacity, outArchive, outSuccess_dev, outSize_dev, outArchiveSize_dev, stream),
                  "floatDecompressReduceCompress");
}

// Reduce-compress with mixed sources: as floatDecompressReduceCompress, source k an archive (sourceKind[k] == 0) or a RAW
// row of exactly outCapacity[i] words of config.floatType (1); `sourceKind` is a HOST array shaped like `in`.
// dgpu_float_reduce_compress_mixed of ../dietgpu_amd.h.
inline void floatDecompressReduceCompressMixed(
    StackDeviceMemory& res, const FloatDecompressConfig& config, bool accumulate, uint32_t numInBatch, uint32_t numSources,
    const void** in, const uint32_t* inBytes, const uint8_t* sourceKind, float** acc, const uint32_t* outCapacity, void** outArchive,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, uint32_t* outArchiveSize_dev, hipStream_t stream) {
  detail::ReduceTemp t(res, stream, outCapacity, numInBatch,
                       [&](uint32_t maxWords) { return dgpu_float_reduce_compress_temp_bytes((uint32_t)config.floatType, numInBatch, maxWords); });
  detail::checkRc(dgpu_float_reduce_compress_mixed(t.ptr, t.bytes, &t.used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                                   accumulate ? 1 : 0, numInBatch, numSources, in, inBytes, sourceKind,
                                                   (void* const*)acc, outCapacity, outArchive, outSuccess_dev, outSize_dev,
                                                   outArchiveSize_dev, stream),
                  "floatDecompressReduceCompressMixed");
}

// Scaled reduce-compress: floatDecompressReduceCompressMixed of fl32(sum * scale): the accumulators hold the scaled sums
// and the archives are those of the scaled sums, rounded once.  `sourceKind` may be null (every source an archive);
// `scale` is finite and not zero, and 1.0f is the unscaled call.  dgpu_float_reduce_compress_scaled of ../dietgpu_amd.h.
inline void floatDecompressReduceCompressScaled(
    StackDeviceMemory& res, const FloatDecompressConfig& config, bool accumulate, uint32_t numInBatch, uint32_t numSources,
    const void** in, const uint32_t* inBytes, const uint8_t* sourceKind, float scale, float** acc, const uint32_t* outCapacity,
    void** outArchive, uint8_t* outSuccess_dev, uint32_t* outSize_dev, uint32_t* outArchiveSize_dev, hipStream_t stream) {
  detail::ReduceTemp t(res, stream, outCapacity, numInBatch,
                       [&](uint32_t maxWords) { return dgpu_float_reduce_compress_temp_bytes((uint32_t)config.floatType, numInBatch, maxWords); });
  detail::checkRc(dgpu_float_reduce_compress_scaled(t.ptr, t.bytes, &t.used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                                    accumulate ? 1 : 0, numInBatch, numSources, in, inBytes, sourceKind, scale,
                                                    (void* const*)acc, outCapacity, outArchive, outSuccess_dev, outSize_dev,
                                                    outArchiveSize_dev, stream),
                  "floatDecompressReduceCompressScaled");
}

// Reduce-compress with the norm outputs: floatDecompressReduceCompressScaled that also leaves, per member, the sum of
// squares (float64) of the finite words of the ARCHIVE -- the sums rounded to config.floatType -- and the number of its
// words that are inf or NaN; a failed member gets 0.0 and 0.  Either may be null.
// dgpu_float_reduce_compress_norm of ../dietgpu_amd.h.
inline void floatReduceCompressNorm(
    StackDeviceMemory& res, const FloatDecompressConfig& config, bool accumulate, uint32_t numInBatch, uint32_t numSources,
    const void** in, const uint32_t* inBytes, const uint8_t* sourceKind, float scale, float** acc, const uint32_t* outCapacity,
    void** outArchive, uint8_t* outSuccess_dev, uint32_t* outSize_dev, uint32_t* outArchiveSize_dev, double* outSumSq_dev,
    uint32_t* outNonFinite_dev, hipStream_t stream) {
  detail::ReduceTemp t(res, stream, outCapacity, numInBatch,
                       [&](uint32_t maxWords) { return dgpu_float_reduce_norm_temp_bytes((uint32_t)config.floatType, numInBatch, maxWords, 1); });
  detail::checkRc(dgpu_float_reduce_compress_norm(t.ptr, t.bytes, &t.used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                                  accumulate ? 1 : 0, numInBatch, numSources, in, inBytes, sourceKind, scale,
                                                  (void* const*)acc, outCapacity, outArchive, outSuccess_dev, outSize_dev,
                                                  outArchiveSize_dev, outSumSq_dev, outNonFinite_dev, stream),
                  "floatReduceCompressNorm");
}

}  // namespace dietgpu
