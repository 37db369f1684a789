// Decode-accumulate in the style of the dietgpu:: mirror (no reference equivalent): float archive i is decoded, every
// word widened to float32 and stored to (accumulate = false) or added into (true) the float32 accumulator out[i] -- the
// float32 reduction of compressed 16-bit gradients without a 16-bit scratch tensor.  Inline on top of
// dgpu_float_decode_accumulate of ../dietgpu_amd.h, where the contract is spelled out.  `inBytes`: the bytes
// available at in[i]; `outCapacity`: float words; the accumulators of one call must not overlap.  The config's
// useChecksum is ignored: a checksum covers the 16-bit words, which never reach memory here.  Uses no temp memory.
#pragma once

#include "GpuFloatCodec.h"

namespace dietgpu {

inline void floatDecompressAccumulate(
    StackDeviceMemory& res, const FloatDecompressConfig& config, bool accumulate, uint32_t numInBatch, const void** in,
    const uint32_t* inBytes, float** out, const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev,
    hipStream_t stream) {
  (void)res;
  size_t used = 0;
  detail::checkRc(dgpu_float_decode_accumulate(nullptr, 0, &used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                                   accumulate ? 1 : 0, numInBatch, in, inBytes, (void* const*)out,
                                                   outCapacity, outSuccess_dev, outSize_dev, stream),
                  "floatDecompressAccumulate");
}

// Scaled decode-accumulate: floatDecompressAccumulate whose every widened word is multiplied by a float32 factor before it
// is stored or added, out[i][k] = [out[i][k] +] fl32(widen(word) * s) -- one IEEE multiply and one IEEE add, never fused.
// `scale_dev`: DEVICE memory holding 1 float (scaleStride 0: one factor for the call) or numInBatch floats (scaleStride
// 1), read when the kernel runs and never by the host -- it may hold any value; null: the host float `scale`, which must
// be finite and not zero, and 1.0f is floatDecompressAccumulate.  dgpu_float_decode_accumulate_scaled of ../dietgpu_amd.h.
inline void floatDecompressAccumulateScaled(
    StackDeviceMemory& res, const FloatDecompressConfig& config, bool accumulate, uint32_t numInBatch, const void** in,
    const uint32_t* inBytes, float** out, const uint32_t* outCapacity, float scale, const float* scale_dev, uint32_t scaleStride,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  (void)res;
  size_t used = 0;
  detail::checkRc(dgpu_float_decode_accumulate_scaled(nullptr, 0, &used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                                      accumulate ? 1 : 0, numInBatch, in, inBytes, (void* const*)out, outCapacity,
                                                      scale, scale_dev, scaleStride, outSuccess_dev, outSize_dev, stream),
                  "floatDecompressAccumulateScaled");
}

// Decode-reduce: numSources archives per accumulator, member-major (source s of member i is in[i * numSources + s], with
// inBytes of the same shape), summed strictly left to right in ONE launch -- bit for bit what numSources successive
// floatDecompressAccumulate calls leave, the first with `accumulate`, the rest with true -- and all or nothing per
// member: outSuccess_dev[i] = 0 leaves out[i] as it was.  dgpu_float_decode_reduce of ../dietgpu_amd.h.
inline void floatDecompressReduce(
    StackDeviceMemory& res, const FloatDecompressConfig& config, bool accumulate, uint32_t numInBatch, uint32_t numSources,
    const void** in, const uint32_t* inBytes, float** out, const uint32_t* outCapacity, uint8_t* outSuccess_dev,
    uint32_t* outSize_dev, hipStream_t stream) {
  (void)res;
  size_t used = 0;
  detail::checkRc(dgpu_float_decode_reduce(nullptr, 0, &used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                           accumulate ? 1 : 0, numInBatch, numSources, in, inBytes, (void* const*)out,
                                           outCapacity, outSuccess_dev, outSize_dev, stream),
                  "floatDecompressReduce");
}

// Decode-reduce with mixed sources: floatDecompressReduce whose source k is an archive (sourceKind[k] == 0) or a RAW row
// of inBytes[k] / wordBytes words of config.floatType (1), word-aligned, widened and added in its place in source order
// -- bit for bit what floatDecompressReduce leaves when the row is replaced by its archive.  `sourceKind` is a HOST
// array shaped like `in`.  dgpu_float_decode_reduce_mixed of ../dietgpu_amd.h.
inline void floatDecompressReduceMixed(
    StackDeviceMemory& res, const FloatDecompressConfig& config, bool accumulate, uint32_t numInBatch, uint32_t numSources,
    const void** in, const uint32_t* inBytes, const uint8_t* sourceKind, float** out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  (void)res;
  size_t used = 0;
  detail::checkRc(dgpu_float_decode_reduce_mixed(nullptr, 0, &used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                                 accumulate ? 1 : 0, numInBatch, numSources, in, inBytes, sourceKind,
                                                 (void* const*)out, outCapacity, outSuccess_dev, outSize_dev, stream),
                  "floatDecompressReduceMixed");
}

// Scaled decode-reduce: floatDecompressReduceMixed that leaves out[i] = fl32(sum * scale) -- one float32 multiply in the
// reduce kernel, on the last source's store; with `accumulate` it covers the old contents too.  `sourceKind` may be null
// (every source an archive); `scale` is finite and not zero, and 1.0f is the unscaled call.
// dgpu_float_decode_reduce_scaled of ../dietgpu_amd.h.
inline void floatDecompressReduceScaled(
    StackDeviceMemory& res, const FloatDecompressConfig& config, bool accumulate, uint32_t numInBatch, uint32_t numSources,
    const void** in, const uint32_t* inBytes, const uint8_t* sourceKind, float scale, float** out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  (void)res;
  size_t used = 0;
  detail::checkRc(dgpu_float_decode_reduce_scaled(nullptr, 0, &used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                                  accumulate ? 1 : 0, numInBatch, numSources, in, inBytes, sourceKind, scale,
                                                  (void* const*)out, outCapacity, outSuccess_dev, outSize_dev, stream),
                  "floatDecompressReduceScaled");
}

// Decode-reduce with the norm outputs: floatDecompressReduceScaled that also leaves, per member, outSumSq_dev[i] = the
// sum of squares (float64) of the finite float32 words it left in out[i] and outNonFinite_dev[i] = the number of words
// that are inf or NaN; a failed or empty member gets 0.0 and 0.  Either may be null.  The tile partials are the call's
// only temp memory and come from `res`.  dgpu_float_decode_reduce_norm of ../dietgpu_amd.h.
inline void floatDecodeReduceNorm(
    StackDeviceMemory& res, const FloatDecompressConfig& config, bool accumulate, uint32_t numInBatch, uint32_t numSources,
    const void** in, const uint32_t* inBytes, const uint8_t* sourceKind, float scale, float** out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, double* outSumSq_dev, uint32_t* outNonFinite_dev, hipStream_t stream) {
  detail::ReduceTemp t(res, stream, outCapacity, numInBatch,
                       [&](uint32_t maxWords) { return dgpu_float_reduce_norm_temp_bytes((uint32_t)config.floatType, numInBatch, maxWords, 0); });
  detail::checkRc(dgpu_float_decode_reduce_norm(t.ptr, t.bytes, &t.used, (uint32_t)config.floatType, config.ansConfig.probBits,
                                                accumulate ? 1 : 0, numInBatch, numSources, in, inBytes, sourceKind, scale,
                                                (void* const*)out, outCapacity, outSuccess_dev, outSize_dev, outSumSq_dev,
                                                outNonFinite_dev, stream),
                  "floatDecodeReduceNorm");
}

}  // namespace dietgpu
