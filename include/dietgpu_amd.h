/*
 * dietgpu_amd.h -- C ABI of the MI355X-native batched rANS / float codec.
 *
 * This is the drop-in boundary for the dietgpu hot path.  The reference has no
 * C ABI (its public API is C++: dietgpu/ans/GpuANSCodec.h and
 * dietgpu/float/GpuFloatCodec.h, taking `StackDeviceMemory&` and
 * `cudaStream_t`); every entry point below names the reference interface it
 * replaces.  Conventions are the reference's own (GpuANSCodec.h:61-341,
 * GpuFloatCodec.h:103-292):
 *
 *   - `in` / `out` / `inSize` / `outCapacity` are HOST arrays holding DEVICE
 *     pointers / sizes; `*_dev` arguments are device memory.
 *   - sizes are BYTES for the ans_* calls and FLOAT WORDS for the float_* calls.
 *   - `outSize_dev`, `outSuccess_dev`, `histogram_dev` may be NULL.
 *   - everything is enqueued on `stream` (a hipStream_t passed as void*); no
 *     host synchronisation happens unless a checksum has to be verified.
 *   - ANS inputs must be 4-byte aligned (kANSRequiredAlignment); float inputs
 *     float-word aligned; compressed buffers 16-byte aligned.  Nothing more is
 *     needed for speed: uncompressed elements at any such address (elements of
 *     a split tensor, rows of a matrix) take the vector paths of every kernel.
 *   - probBits must be 9, 10 or 11.
 *
 * Temporary memory: the reference threads a `StackDeviceMemory&` through every
 * call (dietgpu/utils/StackDeviceMemory.h:141-157).  Here the caller passes a
 * raw device region (`temp_dev`, `tempBytes`; may be NULL/0).  If it is too
 * small the library falls back to hipMalloc + a stderr warning, exactly like
 * the reference's overflow path (StackDeviceMemory.cpp:119-139).  `tempUsed`
 * (nullable) receives the bytes of temp memory the call needed, which is what
 * `StackDeviceMemory::getMaxMemoryUsage()` reports upstream.  The C++ wrappers
 * in include/dietgpu_amd/ re-create the exact `dietgpu::` signatures on top.
 *
 * Return value: 0 on success, a DGPU_ERR_* code otherwise.  Decode calls
 * additionally report a checksum mismatch as DGPU_ERR_CHECKSUM_MISMATCH with
 * the first failing batch index in `*errBatch`; EVERY failing member (upstream
 * pushes each one into `errorInfo`, GpuANSDecode.cuh:581-590,
 * GpuFloatDecompress.cuh:720-733) is available from
 * dgpu_last_checksum_mismatches() (ANSDecodeStatus / FloatDecompressStatus,
 * GpuANSCodec.h:45-59, GpuFloatCodec.h:84-99).
 */
#ifndef DIETGPU_AMD_H
#define DIETGPU_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGPU_OK 0
#define DGPU_ERR_INVALID_ARGUMENT 1
#define DGPU_ERR_HIP 2
#define DGPU_ERR_CHECKSUM_MISMATCH 3

/* FloatType, dietgpu/float/GpuFloatCodec.h:21-26 */
#define DGPU_FLOAT_UNDEFINED 0u
#define DGPU_FLOAT16 1u
#define DGPU_BFLOAT16 2u
#define DGPU_FLOAT32 3u

/* kANSRequiredAlignment / kANSDefaultProbBits, GpuANSCodec.h:16-20 */
#define DGPU_ANS_REQUIRED_ALIGNMENT 4
#define DGPU_ANS_DEFAULT_PROB_BITS 10

const char* dgpu_version(void);
/* Bumped whenever an entry point of this header is removed or changes its meaning.  Code that is built separately
 * against this header (the tensor-op library of this repository, a cgo / JNI binding) compares the value it was compiled
 * with against the library it finds at run time, so that a stale build fails at load instead of inside a call.  An entry
 * point that is only ADDED leaves every existing one as it was and does not move the version: a library without the new
 * symbol fails at load too, by symbol resolution, in anything that links it (dgpu_float_decode_accumulate,
 * dgpu_float_cast_compress, dgpu_float_decode_reduce, dgpu_float_reduce_compress,
 * dgpu_float_reduce_compress_temp_bytes, dgpu_float_rolling_compress, dgpu_float_decode_reduce_mixed,
 * dgpu_float_reduce_compress_mixed, dgpu_float_decode_reduce_scaled, dgpu_float_reduce_compress_scaled,
 * dgpu_float_reduce_norm_temp_bytes, dgpu_float_decode_reduce_norm, dgpu_float_reduce_compress_norm and
 * dgpu_float_decode_scaled were added at version 8, dgpu_float_feedback_compress and
 * dgpu_float_decode_accumulate_scaled after them, dgpu_float_decode_update after those,
 * dgpu_float_stochastic_compress after dgpu_float_decode_update). */
#define DGPU_ABI_VERSION 8u
uint32_t dgpu_abi_version(void);
/* Text of the last error on the calling thread (HIP error string, failed
 * precondition).  The reference aborts through glog CHECK instead. */
const char* dgpu_last_error(void);

/* The batch members whose checksum did not match in the LAST decode call the calling thread made (thread-local,
 * like dgpu_last_error): returns their number and writes up to `cap` of them, ascending batch index, into the
 * arrays that are not NULL.  Replaces the `errorInfo` vector of ANSDecodeStatus / FloatDecompressStatus
 * (GpuANSDecode.cuh:581-590, GpuFloatDecompress.cuh:720-733), which lists every mismatching member. */
uint32_t dgpu_last_checksum_mismatches(int32_t* batchIdx, uint32_t* expected, uint32_t* got, uint32_t cap);

/* ---- size queries -------------------------------------------------------- */
/* getMaxCompressedSize, GpuANSCodec.h:22 / GpuANSEncode.cu:13-25.  Upstream CHECKs the result against INT32_MAX
 * (GpuANSEncode.cu:22), i.e. aborts for inputs of more than 1 717 538 816 bytes; here such a size returns 0 (the
 * C++ mirror aborts like upstream) and the encode entry points reject it with DGPU_ERR_INVALID_ARGUMENT. */
uint32_t dgpu_ans_max_compressed_size(uint32_t uncompressedBytes);
/* getMaxFloatCompressedSize, GpuFloatCodec.h:31 / GpuFloatCompress.cu:23-45 (0 beyond the same guard, which
 * applies to the exponent plane: numFloats bytes) */
uint32_t dgpu_float_max_compressed_size(uint32_t floatType, uint32_t numFloats);
/* Upper bound of temp memory the matching call needs, so a caller can size
 * `temp_dev` once and stay allocation-free (README.md:90-94). */
size_t dgpu_ans_encode_temp_bytes(uint32_t numInBatch, uint32_t maxBytes);
size_t dgpu_ans_decode_temp_bytes(uint32_t numInBatch, uint32_t maxBytes, int probBits);
size_t dgpu_float_compress_temp_bytes(uint32_t floatType, uint32_t numInBatch, uint32_t maxFloats);
size_t dgpu_float_decompress_temp_bytes(uint32_t floatType, uint32_t numInBatch, uint32_t maxFloats, int probBits);

/* ---- rANS encode --------------------------------------------------------- */
/* ansEncodeBatchStride, GpuANSCodec.h:65-98 / GpuANSEncode.cu:27-53 */
int dgpu_ans_encode_batch_stride(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    int probBits, int useChecksum,
    uint32_t numInBatch,
    const void* in_dev, uint32_t inPerBatchSize, uint32_t inPerBatchStride,
    const uint32_t* histogram_dev,
    void* out_dev, uint32_t outPerBatchStride,
    uint32_t* outSize_dev,
    void* stream);

/* ansEncodeBatchPointer, GpuANSCodec.h:100-128 / GpuANSEncode.cu:55-113 */
int dgpu_ans_encode_batch_pointer(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    int probBits, int useChecksum,
    uint32_t numInBatch,
    const void* const* in, const uint32_t* inSize,
    const uint32_t* histogram_dev,
    void* const* out,
    uint32_t* outSize_dev,
    void* stream);

/* ansEncodeBatchSplitSize, GpuANSCodec.h:130-164 / GpuANSEncode.cu:115-179 */
int dgpu_ans_encode_batch_split_size(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    int probBits, int useChecksum,
    uint32_t numInBatch,
    const void* in_dev, const uint32_t* inSplitSizes,
    const uint32_t* histogram_dev,
    void* out_dev, uint32_t outStride,
    uint32_t* outSize_dev,
    void* stream);

/* ---- rANS decode --------------------------------------------------------- */
/* What the entry points WITHOUT input sizes may read (the reference's contract, made explicit): up to
 * dgpu_ans_max_compressed_size(outCapacity) / dgpu_float_max_compressed_size(type, outCapacity) bytes from every input
 * pointer -- the size of the buffer an encoder was given for an element of that capacity (GpuANSCodec.h:24-26,
 * GpuFloatCodec.h:54-57).  Inside that extent every format invariant is checked before it is followed; the decoders
 * request the probability table and (float archives, once the float header has been checked) the block descriptor
 * and lane states of the blocks the header implies in the same round trip as the ANS header, i.e. before that header
 * has been validated.  Callers that hold archives in buffers SMALLER than that -- received, truncated to their size --
 * use the *_bounded entry points below, which read nothing beyond the bytes they are told exist. */
/* ansDecodeBatchStride, GpuANSCodec.h:170-226 / GpuANSDecode.cu:20-45 */
int dgpu_ans_decode_batch_stride(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    int probBits, int useChecksum,
    uint32_t numInBatch,
    const void* in_dev, uint32_t inPerBatchStride,
    void* out_dev, uint32_t outPerBatchStride, uint32_t outPerBatchCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev,
    void* stream, int32_t* errBatch);

/* ansDecodeBatchPointer, GpuANSCodec.h:228-263 / GpuANSDecode.cu:47-120 */
int dgpu_ans_decode_batch_pointer(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    int probBits, int useChecksum,
    uint32_t numInBatch,
    const void* const* in,
    void* const* out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev,
    void* stream, int32_t* errBatch);

/* ansDecodeBatchSplitSize, GpuANSCodec.h:265-304 / GpuANSDecode.cu:122-193 */
int dgpu_ans_decode_batch_split_size(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    int probBits, int useChecksum,
    uint32_t numInBatch,
    const void* const* in,
    void* out_dev, const uint32_t* outSplitSizes,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev,
    void* stream, int32_t* errBatch);

/* ---- rANS info ----------------------------------------------------------- */
/* ansGetCompressedInfo, GpuANSCodec.h:310-324 / GpuANSInfo.cu:13-35 (host
 * array of device pointers) */
int dgpu_ans_get_compressed_info(
    void* temp_dev, size_t tempBytes,
    const void* const* in, uint32_t numInBatch,
    uint32_t* outSizes_dev, uint32_t* outChecksum_dev, void* stream);
/* ansGetCompressedInfoDevice, GpuANSCodec.h:326-341 / GpuANSInfo.cu:37-49 */
int dgpu_ans_get_compressed_info_device(
    const void* const* in_dev, uint32_t numInBatch,
    uint32_t* outSizes_dev, uint32_t* outChecksum_dev, void* stream);

/* ---- float codec --------------------------------------------------------- */
/* floatCompress, GpuFloatCodec.h:103-141 / GpuFloatCompress.cu:47-101 */
int dgpu_float_compress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch,
    const void* const* in, const uint32_t* inSize,
    void* const* out,
    uint32_t* outSize_dev,
    void* stream);

/* floatCompressSplitSize, GpuFloatCodec.h:143-178 / GpuFloatCompress.cu:103-159 */
int dgpu_float_compress_split_size(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch,
    const void* in_dev, const uint32_t* inSplitSizes,
    void* out_dev, uint32_t outStride,
    uint32_t* outSize_dev,
    void* stream);

/* floatDecompress, GpuFloatCodec.h:184-218 / GpuFloatDecompress.cu:22-115 */
int dgpu_float_decompress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch,
    const void* const* in,
    void* const* out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev,
    void* stream, int32_t* errBatch);

/* floatDecompressSplitSize, GpuFloatCodec.h:220-258 / GpuFloatDecompress.cu:117-179 */
int dgpu_float_decompress_split_size(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch,
    const void* const* in,
    void* out_dev, const uint32_t* outSplitSizes,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev,
    void* stream, int32_t* errBatch);

/* ---- decode with known input sizes (no upstream equivalent) -------------------
 * The reference's decode API carries no compressed sizes (GpuANSCodec.h:228-304,
 * GpuFloatCodec.h:184-258): an archive that was cut short is followed past its buffer.
 * These variants take `inBytes` (HOST array, bytes available at in[i]); an archive whose
 * header claims more is reported through outSuccess and not read.  The tensor-level
 * ops (decompress_data*, DietGpu.cpp:530-911), which know every input tensor's size,
 * go through them. */
int dgpu_ans_decode_batch_pointer_bounded(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits, int useChecksum,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes,
    void* const* out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream, int32_t* errBatch);
int dgpu_ans_decode_batch_split_size_bounded(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits, int useChecksum,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes,
    void* out_dev, const uint32_t* outSplitSizes,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream, int32_t* errBatch);
int dgpu_float_decompress_bounded(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes,
    void* const* out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream, int32_t* errBatch);
int dgpu_float_decompress_split_size_bounded(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes,
    void* out_dev, const uint32_t* outSplitSizes,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream, int32_t* errBatch);

/* ---- ranged decode (no upstream equivalent) ----------------------------------------
 * Decodes blocks [firstBlock[i], firstBlock[i] + numBlocks[i]) of archive i -- a block is the format's 4096 symbols
 * (bytes / float words) -- without reading or decoding the rest: block firstBlock + k goes to out[i] + k * 4096 words,
 * so out[i] holds the range, and `outCapacity` (bytes for ans, float words for float) is that buffer's.  Pointer-array
 * batches that always take `inBytes`, as the *_bounded calls above.  firstBlock / numBlocks are HOST arrays;
 * numBlocks[i] == UINT32_MAX means "to the end of the element", and a range that runs past the end is clipped to it.
 *   - outSize_dev[i] = min(total, (firstBlock + numBlocks) * 4096) - firstBlock * 4096 words (bytes).
 *   - outSuccess_dev[i] = 0 and nothing written when a header check fails (as for a whole decode), firstBlock * 4096 >
 *     total, the clipped range does not fit outCapacity[i], or a block descriptor OF THE RANGE is malformed.  A range
 *     that begins exactly at the end is empty and succeeds.  Descriptors outside the range are not looked at.
 *   - numBlocks[i] == 0: nothing of archive i is read; size 0, success 1.
 *   - outCapacity[i] must not exceed 0xfffff000 (whole blocks below 4 Gi words): DGPU_ERR_INVALID_ARGUMENT otherwise.
 *   - There is no useChecksum: a checksum covers the whole element and cannot be verified from a part of it.  Archives
 *     written with one decode normally; the checksum is ignored.
 *   - Of the archive only the headers, the probability table and the descriptors, lane states, compressed words and
 *     non-compressed plane slices of the range's blocks are read.  One kernel geometry per call, from its largest range.
 *   - No temp memory is used (*tempUsed = 0) and nothing synchronises: capturable into a HIP graph under the same
 *     conditions as the other pointer-array decode calls (the arrays resident from an earlier identical call). */
int dgpu_ans_decode_batch_pointer_range(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes,
    const uint32_t* firstBlock, const uint32_t* numBlocks,
    void* const* out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream);
int dgpu_float_decompress_range(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes,
    const uint32_t* firstBlock, const uint32_t* numBlocks,
    void* const* out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream);

/* ---- decode-accumulate (no upstream equivalent) --------------------------------------
 * Decodes float archive i, widens every word to float32 and stores it to (accumulate == 0) or adds it into
 * (accumulate == 1) the float32 accumulator out[i] -- the reduction of compressed 16-bit gradients in float32 without a
 * 16-bit scratch tensor, and (accumulate == 0) the decompression of a 16-bit archive straight into float32.
 * Pointer-array batch that always takes `inBytes`, as the *_bounded calls above; `outCapacity` is in float words.
 *   - Widening is exact: float16 converts (denormals included), bfloat16 is word << 16, float32 passes through.  The
 *     sum is ONE IEEE float32 add per word, round to nearest even, denormals kept, not contracted with anything; with
 *     accumulate == 0 the accumulator is not read (no memset is needed before the first source of a sum) and the bits
 *     of the widened word are stored as they are.
 *   - floatType must be DGPU_FLOAT16, DGPU_BFLOAT16 or DGPU_FLOAT32 (there is no raw-byte form), accumulate 0 or 1,
 *     in[i] 16-byte aligned, out[i] 4-byte aligned, outCapacity[i] <= 0xfffff000: DGPU_ERR_INVALID_ARGUMENT otherwise,
 *     before anything is enqueued.  The accumulators of the members of one call MUST NOT overlap.
 *   - outSize_dev[i], outSuccess_dev[i] and every header and descriptor check are those of a whole bounded decode.  A
 *     member that fails (outSuccess_dev[i] = 0) leaves its accumulator untouched and does not disturb the others.
 *   - There is no useChecksum: a checksum covers the 16-bit (32-bit) words of the element, which never reach memory
 *     here.  Archives written with one decode normally; the checksum is ignored.
 *   - One kernel geometry per call, from its largest capacity.
 *   - No temp memory is used (*tempUsed = 0) and nothing synchronises: capturable into a HIP graph under the same
 *     conditions as the other pointer-array decode calls (the arrays resident from an earlier identical call). */
int dgpu_float_decode_accumulate(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes,
    void* const* out /* float32 */, const uint32_t* outCapacity /* float words */,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream);

/* ---- scaled decode-accumulate (no upstream equivalent) --------------------------------
 * dgpu_float_decode_accumulate whose every widened word is multiplied by a float32 factor before it is stored or added:
 * out = [out +] s * x in float32, with s read by the kernel from device memory.  It is the decode of the final
 * all-gather of a compressed all-reduce into a float32 gradient buffer with the clip coefficient applied, gradient
 * accumulation over micro-batches (accumulate == 1), and with s = -lr * coef the SGD update of float32 master weights
 * straight from the archive.
 *   - For every decoded word w of member i with factor s_i:  p = fl32(widen(w) * s_i);  out[i][k] = accumulate ?
 *     fl32(out[i][k] + p) : p.  Widening is exact, as in dgpu_float_decode_accumulate (float32 archives: the identity).
 *     ONE IEEE float32 multiply and ONE IEEE float32 add, each rounded once to nearest even, denormals kept, never fused
 *     into an FMA: bit for bit what decode-accumulate into a scratch, a float32 multiply by the factor and a float32 add
 *     compose to.  With accumulate == 0 the accumulator is not read.
 *   - The factor: scale_dev != NULL points at DEVICE memory, 4-byte aligned, of 1 float (scaleStride == 0: one factor
 *     for the call) or numInBatch floats (scaleStride == 1: member i takes scale_dev[i]).  It is read when the kernel
 *     runs and never by the host, so it may be the result of work enqueued earlier on the stream, and a captured call
 *     follows the value the memory holds at each replay.  It may hold ANY value -- 0, an infinity, a NaN, 1 -- and the
 *     arithmetic above is the contract for all of them: a device factor of 1 multiplies (a signalling NaN leaves
 *     quiet).  scale_dev == NULL: the host float `scale`, which must be finite and not zero.  A host float of exactly
 *     1.0f IS dgpu_float_decode_accumulate (the call forwards to it): with accumulate == 0 a signalling NaN of a float32
 *     archive keeps its bits.
 *   - Everything else is dgpu_float_decode_accumulate's: every header and descriptor check, outSuccess_dev[i] and
 *     outSize_dev[i]; a member that fails (outSuccess_dev[i] = 0) keeps every bit of its accumulator and does not
 *     disturb the others; a capacity larger than the element leaves the words behind the element untouched; the
 *     accumulators are 4-byte aligned and those of one call MUST NOT overlap; there is no useChecksum (a checksum in
 *     the archive is ignored); one kernel geometry per call, from its largest capacity.
 *   - floatType must be DGPU_FLOAT16, DGPU_BFLOAT16 or DGPU_FLOAT32, probBits 9, 10 or 11, accumulate 0 or 1,
 *     scaleStride 0 or 1, scale_dev 4-byte aligned, a host scale finite and not zero, no array null when
 *     numInBatch > 0, in[i] 16-byte aligned, out[i] 4-byte aligned, outCapacity[i] <= 0xfffff000:
 *     DGPU_ERR_INVALID_ARGUMENT with a dgpu_last_error() text otherwise, before anything is enqueued.  An empty batch
 *     returns 0.
 *   - No temp memory is used (*tempUsed = 0) and nothing synchronises: capturable into a HIP graph under the same
 *     conditions as the other pointer-array decode calls (the arrays resident from an earlier identical call). */
int dgpu_float_decode_accumulate_scaled(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes,
    void* const* out /* float32 */, const uint32_t* outCapacity /* float words */,
    float scale, const float* scale_dev /* nullable: the host float is used */, uint32_t scaleStride /* 0 or 1 */,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream);

/* ---- scaled decompress (no upstream equivalent) ---------------------------------------
 * dgpu_float_decompress_bounded (useChecksum = 0) that multiplies every word by a float32 factor before it stores it:
 * the decode of the final all-gather of a compressed all-reduce applies the clip coefficient, which is known only
 * after the reduce, without a second pass over the tensor and without the host ever reading the coefficient.
 *   - For member i with factor s and the archive's type T: out[i][k] = round_T(fl32(widen(word_k) * s)).  Widening is
 *     exact, as in dgpu_float_decode_accumulate; ONE IEEE float32 multiply, round to nearest even, denormals kept, not
 *     contracted; ONE rounding to T as in dgpu_float_cast_compress (nearest even, float16 denormals produced, overflow
 *     to infinity, the sign of zero kept); float32 archives store the product.  A NaN product is stored as a quiet NaN
 *     of T, never as an infinity; its sign and payload are the platform's.
 *   - The factor: scale_dev != NULL points at DEVICE memory, 4-byte aligned, of 1 float (scaleStride == 0: one factor
 *     for the call) or numInBatch floats (scaleStride == 1: member i takes scale_dev[i]).  It is read when the kernel
 *     runs and never by the host, so it may be the result of work enqueued earlier on the stream, and a captured call
 *     follows the value the memory holds at each replay.  It may hold ANY value, and the arithmetic above is the
 *     contract for all of them (0 gives signed zeros for finite words; +-inf gives +-inf for non-zero words and NaN for
 *     zeros; 1 gives back the bits of every word that is not a NaN).  scale_dev == NULL: the host float `scale`, which
 *     must be finite and not zero.
 *   - Everything else is the whole bounded float decode: the archive checks, outSuccess_dev / outSize_dev, a capacity
 *     larger than the element leaves the words behind the element untouched, a member of another float type or with a
 *     malformed archive gets outSuccess_dev[i] = 0 and does not disturb the others.
 *   - floatType must be DGPU_FLOAT16, DGPU_BFLOAT16 or DGPU_FLOAT32, probBits 9, 10 or 11, scaleStride 0 or 1,
 *     in[i] 16-byte aligned, out[i] as dgpu_float_decompress_bounded takes it, outCapacity[i] <= 0xfffff000, no array
 *     null when numInBatch > 0: DGPU_ERR_INVALID_ARGUMENT otherwise, before anything is enqueued.
 *   - There is no useChecksum: a checksum covers the stored words of the original tensor, which this call does not
 *     leave.  Archives written with one decode normally; the checksum is ignored.
 *   - One kernel geometry per call, from its largest capacity (single-block members run on the 4-block tiles).
 *   - No temp memory is used (*tempUsed = 0) and nothing synchronises: capturable into a HIP graph under the same
 *     conditions as the other pointer-array decode calls (the arrays resident from an earlier identical call). */
int dgpu_float_decode_scaled(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes,
    void* const* out, const uint32_t* outCapacity /* float words */,
    float scale, const float* scale_dev /* nullable: the host float is used */, uint32_t scaleStride /* 0 or 1 */,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream);

/* ---- decode-update (no upstream equivalent) -------------------------------------------
 * Decodes 16-bit float archives, multiplies every word by a float32 factor, adds it to a 16-bit tensor OF THE ARCHIVE'S
 * TYPE and rounds the sum STOCHASTICALLY back to that type: with s = -lr * coef the SGD update of bfloat16 / float16
 * parameters that have no float32 master copy, straight from the final all-gather of a compressed all-reduce.  One
 * kernel: 2 bytes read and 2 written per word beside the archive.
 *   For decoded word w_k (index k within member i), factor s_i and tensor word t_k = out[i][k]:
 *   1. p = fl32(widen(w_k) * s_i).  Widening is exact; ONE IEEE float32 multiply, as in
 *      dgpu_float_decode_accumulate_scaled.
 *   2. v = accumulate ? fl32(widen(t_k) + p) : p.  ONE IEEE float32 add, never fused with the multiply.  With
 *      accumulate == 0 the tensor is not read.
 *   3. out[i][k] = sround_T(bits(v), r16(S, firstMember + i, k)), with S = seed_dev ? *seed_dev : seed.
 *   - sround_T(x, r) works on the float32 bits x with a 16-bit number r.  Let a = x & 0x7fffffff and
 *     sign = (x >> 16) & 0x8000.  A NaN (a > 0x7f800000) becomes the canonical quiet NaN of T (sign | 0x7fc0 for
 *     bfloat16, sign | 0x7e00 for float16); the sign of a NaN that the arithmetic produced is unspecified.
 *     bfloat16: (x + r) >> 16.
 *     float16: u = a - 0x38000000 when a >= 0x38800000; otherwise u = floor(|v| * 2^37), that is m >> (113 - max(e, 1))
 *     with e = a >> 23, m = (a & 0x7fffff) | (e ? 0x800000 : 0), and 0 once the shift reaches 32.
 *     h = min((u + (r >> 3)) >> 13, 0x7c00); the result is sign | h.
 *   - So: the result is the neighbour of v toward zero or the next one away from zero, "away" with probability
 *     remainder / unit -- exact to 2^-16 for bfloat16 and to 2^-13 for float16; for float16-denormal results the
 *     truncation of u adds less than 2^-13 of a unit.  A value that T represents never moves; infinities stay
 *     infinities; a finite v beyond T's largest value can round to infinity; r = 0 is truncation.
 *   - r16(S, j, k), with mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (mod 2^32):
 *     base = mix32(mix32(lo32(S) + 0x9E3779B9) ^ hi32(S));  key_j = mix32(base + j * 0x85EBCA6B);
 *     bits = mix32(key_j ^ (k >> 1));  r16 = the low half of bits for even k, the high half for odd k.
 *     The random bits are a pure function of (seed, member, word index): every replica that decodes the same archives
 *     with the same seed holds the same parameter bits, whatever the kernel geometry, the dispatch order, the
 *     dgpu_debug_set_* knobs or the alignment of out[i]; firstMember lets a batch split over several calls draw the
 *     bits of the whole batch.
 *   - The factor is dgpu_float_decode_scaled's: scale_dev != NULL points at DEVICE memory, 4-byte aligned, of 1 float
 *     (scaleStride == 0) or numInBatch floats (scaleStride == 1), read when the kernel runs and never by the host; it
 *     may hold ANY value.  scale_dev == NULL: the host float `scale`, which must be finite and not zero.
 *   - seed_dev != NULL points at DEVICE memory, 8-byte aligned, of one uint64_t that the kernel reads when it runs: a
 *     captured call advances the rounding by advancing that word.  seed_dev == NULL: the host `seed`.
 *   - Every archive check of dgpu_float_decode_scaled applies; outSuccess_dev[i] and outSize_dev[i] behave as there.  A
 *     member that fails (outSuccess_dev[i] = 0: another float type, a malformed or truncated archive, one that does not
 *     fit) keeps EVERY bit of its tensor and does not disturb the others.  Words behind the element stay untouched and
 *     no byte outside [out[i], out[i] + size) is written: tensors laid side by side in one buffer, with odd sizes, are
 *     a legal call.  out[i] is 2-byte aligned; the tensors of one call must not overlap each other or the archives.
 *   - floatType (of the archives AND of the tensors) must be DGPU_FLOAT16 or DGPU_BFLOAT16 -- DGPU_FLOAT32 is rejected --
 *     probBits 9, 10 or 11, accumulate 0 or 1, scaleStride 0 or 1, scale_dev 4-byte aligned, seed_dev 8-byte aligned, a
 *     host scale finite and not zero, no array null when numInBatch > 0, in[i] 16-byte aligned, out[i] 2-byte aligned,
 *     outCapacity[i] <= 0xfffff000: DGPU_ERR_INVALID_ARGUMENT with a dgpu_last_error() text otherwise, before anything
 *     is enqueued.  An empty batch returns 0.  There is no checksum (one in the archive is ignored).
 *   - One kernel geometry per call, from its largest capacity (single-block members run on the 4-block tiles).
 *   - No temp memory is used -- the call has no temp-memory parameters -- and nothing synchronises: capturable into a
 *     HIP graph under the same conditions as the other pointer-array decode calls (the arrays resident from an earlier
 *     identical call). */
int dgpu_float_decode_update(
    uint32_t floatType /* of the archives AND of the tensors: DGPU_FLOAT16 or DGPU_BFLOAT16 */, int probBits,
    int accumulate, uint32_t numInBatch, const void* const* in, const uint32_t* inBytes,
    void* const* out /* 16-bit words of floatType */, const uint32_t* outCapacity /* words */,
    float scale, const float* scale_dev /* nullable */, uint32_t scaleStride /* 0 or 1 */,
    uint64_t seed, const uint64_t* seed_dev /* nullable */, uint32_t firstMember,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream);

/* ---- decode-reduce (no upstream equivalent) ------------------------------------------
 * dgpu_float_decode_accumulate with numSources archives per accumulator, summed in ONE launch: the receiving side of a
 * compressed reduce-scatter, where `world` compressed rows belong to one float32 shard.
 *   - Layout: member-major.  Source s of member i is in[i * numSources + s], with inBytes[i * numSources + s] bytes
 *     available; out, outCapacity, outSuccess_dev and outSize_dev have numInBatch entries.
 *   - Result: strictly left to right, one IEEE float32 add (__fadd_rn) per word and source.  accumulate == 1:
 *     out[i] = ((acc + x0) + x1) + ... + x(S-1).  accumulate == 0: out[i] = (x0 + x1) + ... + x(S-1); the widened bits of
 *     x0 are stored as they are and the accumulator is never read.  Widening as in dgpu_float_decode_accumulate.  Bit
 *     for bit what numSources successive dgpu_float_decode_accumulate calls leave, the first with `accumulate`, the
 *     rest with 1.
 *   - All or nothing per member: outSuccess_dev[i] = 1 only if EVERY source of member i passes every check of a bounded
 *     decode-accumulate against outCapacity[i] and its own inBytes (float header, ANS header, probBits, float type,
 *     block count, every block descriptor, pdf sum, the archive inside inBytes) and all numSources headers state the
 *     same word count.  Otherwise outSuccess_dev[i] = 0, out[i] keeps every bit it had (also with accumulate == 0), and
 *     the other members are not disturbed.
 *   - outSize_dev[i]: the word count the header of source 0 states, as a decode of source 0 alone reports it (0 if
 *     source 0 has fewer bytes than a header).
 *   - floatType must be DGPU_FLOAT16, DGPU_BFLOAT16 or DGPU_FLOAT32, accumulate 0 or 1, probBits 9, 10 or 11,
 *     1 <= numSources <= 64, numInBatch * numSources <= 65535, in[...] 16-byte aligned, out[i] 4-byte aligned,
 *     outCapacity[i] <= 0xfffff000, no array null when numInBatch > 0: DGPU_ERR_INVALID_ARGUMENT otherwise, with a
 *     dgpu_last_error() text, before anything is enqueued.  An empty batch returns 0 with *tempUsed = 0.  The
 *     accumulators of different members MUST NOT overlap; sources may alias each other.
 *   - numSources == 1 IS dgpu_float_decode_accumulate (the call forwards to it).
 *   - No useChecksum (see above).  One kernel geometry per call, from its largest capacity.
 *   - No temp memory is used (*tempUsed = 0) and nothing synchronises: capturable into a HIP graph under the same
 *     conditions as the other pointer-array decode calls (the arrays resident from an earlier identical call). */
int dgpu_float_decode_reduce(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources,
    const void* const* in /* [numInBatch * numSources] */, const uint32_t* inBytes /* same shape */,
    void* const* out /* float32, [numInBatch] */, const uint32_t* outCapacity /* float words, [numInBatch] */,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream);

/* ---- cast-compress (no upstream equivalent) -------------------------------------------
 * Compresses float32 element i into an ordinary float16 / bfloat16 archive: every word is rounded to `floatType` in
 * registers, by the histogram pass and by the encoder alike, and the archive is byte for byte what dgpu_float_compress
 * (useChecksum = 0) writes for the already-rounded tensor -- every decoder of this header reads it.  The sending side
 * of a compressed exchange whose values are float32 (master weights, gradient accumulators, the float32 sums of
 * dgpu_float_decode_accumulate) without a 16-bit scratch tensor and the cast kernel that fills it.
 *   - The rounding, on the float32 bits x: bfloat16 is (x + 0x7fff + ((x >> 16) & 1)) >> 16 -- round to nearest even,
 *     float32 denormals are not flushed, overflow goes to infinity; float16 is the IEEE conversion, round to nearest
 *     even, float16 denormals produced, |v| >= 65520 -> infinity, the sign of zero kept.  A NaN of either sign and any
 *     payload becomes the canonical quiet NaN with the sign kept (sign | 0x7fc0, sign | 0x7e00): never an infinity.
 *   - floatType is the type of the ARCHIVE: DGPU_FLOAT16 or DGPU_BFLOAT16 (float32 -> float32 is dgpu_float_compress);
 *     in[i] 4-byte aligned, out[i] 16-byte aligned with room for dgpu_float_max_compressed_size(floatType, inSize[i]),
 *     probBits 9 / 10 / 11, numInBatch <= 65535, inSize[i] (words) within the size guard of dgpu_float_compress:
 *     DGPU_ERR_INVALID_ARGUMENT otherwise, before anything is enqueued.  An empty batch returns 0, *tempUsed = 0.
 *   - There is no useChecksum: a checksum covers the 16-bit words, which never reach memory here.
 *   - Temp memory: dgpu_float_compress_temp_bytes(floatType, numInBatch, max inSize).  Stride detection, parameter
 *     cache, work lists, size classes and graph capture are those of dgpu_float_compress; elements of a single block
 *     run on the 2-block tiles (there is no cast form of the single-block kernels). */
int dgpu_float_cast_compress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    uint32_t floatType /* of the ARCHIVE: DGPU_FLOAT16 or DGPU_BFLOAT16 */, int probBits,
    uint32_t numInBatch, const void* const* in /* float32 */, const uint32_t* inSize /* words */,
    void* const* out, uint32_t* outSize_dev, void* stream);

/* ---- feedback cast-compress (no upstream equivalent) ------------------------------------
 * dgpu_float_cast_compress with error feedback: the sender of a compressed exchange of float32 gradients keeps a float32
 * residual per tensor, the call adds it before the rounding and stores the new rounding error back, so that what one
 * step's rounding drops reaches the wire in a later step.  For word k of element i, on the float32 bits:
 *   1. residualIn given: v = x[k] + e[k] -- ONE IEEE float32 add, round to nearest even, denormals kept, not
 *      contracted.  residualIn == NULL (the ARRAY: no residual yet): v = x[k], NO add -- -0.0f keeps its sign and a
 *      signalling NaN reaches the rounding as it is (a zero-filled residual is not the same thing: -0 + +0 = +0).
 *      Where both x[k] and e[k] are NaNs, or the add is invalid (inf - inf), v is a NaN whose sign is unspecified.
 *   2. q = the rounding of dgpu_float_cast_compress applied to v (nearest even, float16 denormals produced, overflow to
 *      infinity, every NaN to the canonical quiet NaN with its sign).
 *   3. residualOut[i][k] = v - widen(q) when q is finite -- exact, so its rounding mode never shows ((-0) - (-0) is
 *      +0) -- and +0.0f (bits 0) when q is an infinity or a NaN: one overflowing step does not poison the residual for
 *      good.  Whether to take such a step remains the caller's decision, as elsewhere.
 *   4. out[i] / outSize_dev[i] are byte for byte what dgpu_float_cast_compress(floatType, probBits) writes for the
 *      float32 tensor v: an ordinary archive that every decoder of this header reads.
 *   - In place: residualOut[i] == residualIn[i], exactly, is allowed and is the intended use -- one buffer per tensor.
 *     Any other overlap among in, residualIn, residualOut and out, within or across members, is invalid
 *     (DGPU_ERR_INVALID_ARGUMENT).  `in` is never written.
 *   - Exactly inSize[i] words of residualOut[i] are written: no byte before or behind them is touched, an empty element
 *     writes nothing.
 *   - in[i], residualIn[i] and residualOut[i] are 4-byte aligned and congruent to each other modulo 16 (a residual laid
 *     out like its tensor always is); out[i] 16-byte aligned with room for dgpu_float_max_compressed_size(floatType,
 *     inSize[i]).  probBits 9 / 10 / 11, numInBatch <= 65535, inSize[i] within the size guard, floatType DGPU_FLOAT16 or
 *     DGPU_BFLOAT16, residualOut not NULL when numInBatch > 0, no entry of a given array NULL:
 *     DGPU_ERR_INVALID_ARGUMENT otherwise, with a dgpu_last_error() text, before anything is enqueued.  An empty batch
 *     returns 0 with *tempUsed = 0.
 *   - No checksum, for dgpu_float_cast_compress's reason.  Temp memory: within
 *     dgpu_float_compress_temp_bytes(floatType, numInBatch, max inSize).
 *   - The host routes are dgpu_float_cast_compress's: stride detection (the residual arrays included), parameter cache
 *     (the residual pointers are part of the resident block and of its key), work lists, size classes, both dispatch
 *     forms, no host synchronisation, capturable into a HIP graph after one identical warm call; single-block elements
 *     run on the 2-block tiles. */
int dgpu_float_feedback_compress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    uint32_t floatType /* of the ARCHIVE: DGPU_FLOAT16 or DGPU_BFLOAT16 */, int probBits,
    uint32_t numInBatch, const void* const* in /* float32 */, const uint32_t* inSize /* words */,
    const void* const* residualIn /* float32, [numInBatch]; the ARRAY may be NULL: no residual yet */,
    void* const* residualOut /* float32, [numInBatch], required */,
    void* const* out, uint32_t* outSize_dev, void* stream);

/* ---- stochastic cast-compress (no upstream equivalent) ----------------------------------
 * dgpu_float_cast_compress whose every rounding is STOCHASTIC: the sender of a compressed exchange of float32 gradients
 * puts an UNBIASED 16-bit word on the wire without keeping a residual -- what round-to-nearest drops every step, and
 * drops the same way on every rank, is here kept in expectation.  The histogram pass and the encoder round every word in
 * registers and arrive at the same word, because the random bits are a pure function of (seed, member, word index).
 *   - out[i] / outSize_dev[i] are byte for byte what dgpu_float_compress(useChecksum = 0) writes for the 16-bit tensor
 *     q[k] = sround_T(bits(x[k]), r16(S, firstMember + i, k)), k the word's index within element i, with sround_T and
 *     r16 exactly as stated under dgpu_float_decode_update, S = seed_dev ? *seed_dev : seed and firstMember + i taken
 *     modulo 2^32.  The same (S, member, k) draws the same bits in both calls.
 *   - So, as there: a value that T represents never moves; an infinity stays an infinity; a NaN becomes the canonical
 *     quiet NaN with its sign; a finite value beyond T's largest can round to infinity.  The archive is an ordinary
 *     one that every decoder of this header reads.  The result does not depend on the kernel geometry, the dispatch
 *     form, the dgpu_debug_set_* knobs or the alignment of in[i]; firstMember lets a batch split over several calls
 *     draw the bits of the whole batch.  `in` is never written.
 *   - seed_dev != NULL points at DEVICE memory, 8-byte aligned, of one uint64_t.  The kernels read it when they run and
 *     the host never reads it.  BOTH kernels of the call read it, so it must not be written between them: a writer
 *     enqueued earlier on the same stream is fine, one on another stream must be ordered before or after the whole
 *     call.  A captured call follows the word at each replay.  seed_dev == NULL: the host `seed`.
 *   - floatType is the type of the ARCHIVE: DGPU_FLOAT16 or DGPU_BFLOAT16 -- DGPU_FLOAT32 is rejected; in[i] 4-byte
 *     aligned, out[i] 16-byte aligned with room for dgpu_float_max_compressed_size(floatType, inSize[i]), probBits
 *     9 / 10 / 11, numInBatch <= 65535, inSize[i] (words) within the size guard of dgpu_float_compress, no array null
 *     when numInBatch > 0, seed_dev 8-byte aligned: DGPU_ERR_INVALID_ARGUMENT with a dgpu_last_error() text otherwise,
 *     before anything is enqueued.  An empty batch returns 0.  There is no checksum, for dgpu_float_cast_compress's
 *     reason.
 *   - The call has no temp-memory parameters: its temporaries (partial histograms, tables, descriptors, claim words,
 *     spill slots) come from the stream's library-owned slab (dgpu_release_stream_state).  Nothing synchronises.
 *   - The host routes are dgpu_float_cast_compress's, and the call is planned as that call: stride detection,
 *     parameter cache (the seed, seed_dev and firstMember are kernel arguments, not part of the resident block: calls
 *     that differ only in them share it), work lists, size classes, both dispatch forms; capturable into a HIP graph
 *     after one identical warm call; single-block elements run on the 2-block tiles. */
int dgpu_float_stochastic_compress(
    uint32_t floatType /* of the ARCHIVE: DGPU_FLOAT16 or DGPU_BFLOAT16 */, int probBits,
    uint32_t numInBatch, const void* const* in /* float32 */, const uint32_t* inSize /* words */,
    uint64_t seed, const uint64_t* seed_dev /* nullable */, uint32_t firstMember,
    void* const* out, uint32_t* outSize_dev, void* stream);

/* ---- rolling-table compress (no upstream equivalent) ------------------------------------
 * (Named like its siblings dgpu_float_cast_compress and dgpu_float_reduce_compress: the call is a compress with a
 * qualifier in front.)
 * dgpu_float_compress / dgpu_float_cast_compress for tensors that come back step after step (gradient buckets, weight
 * shards): the probability table of this call is made from the exponent counts of the LAST call, so no histogram pass
 * reads the input, and the encoder counts the exponent bytes it codes, which leaves the counts for the NEXT call.
 *   - countsIn_dev / countsOut_dev: device arrays [numInBatch][256] of uint32, 4-byte aligned, either may be NULL.
 *     Both NULL: the call forwards to dgpu_float_compress(useChecksum = 0) / dgpu_float_cast_compress.
 *   - countsOut_dev: after the call countsOut_dev[i][s] is the exact number of words of element i whose exponent byte
 *     -- the byte the format entropy-codes: w >> 8 for float16, bits 14..7 for bfloat16, of the ROUNDED word when
 *     sourceFloat32 -- is s.  A row sums to inSize[i]; an empty element's is 256 zeros.  The library zeroes the rows
 *     itself (nothing is required of what the buffer held) and the encoder adds to them while it codes: the counting
 *     form of the tiled encoder, persistent workgroups on tiles of 2, 4 or 8 blocks whatever
 *     dgpu_debug_set_encoder_dispatch says; elements of a single block run on the 2-block tiles.
 *   - countsIn_dev NULL: the histogram pass runs and the archive is byte for byte the plain call's.
 *   - countsIn_dev given: no histogram kernel runs.  Element i is coded with the table the library's normalisation
 *     yields for c'[s] = min(max(countsIn_dev[i][s], 1), inSize[i]) against a total of inSize[i].  Every symbol then
 *     has a probability >= 1: no element can fail whatever the counts are (stale, of other data, garbage), and the
 *     archive is an ordinary float archive of that table, which every decoder reads.  Only its SIZE depends on how well
 *     the counts fit -- and it is never quite the plain call's: the symbols the data does not use keep a probability
 *     of 2^-probBits each (measured at probBits 10 on N(0, 1) data: bfloat16 archives 4.8 % larger, float16 1.6 %).  (dgpu_ans_encode_* with histogram_dev keep failing data their histogram does not cover.)
 *   - countsIn_dev == countsOut_dev, exactly, is allowed and is the intended use: one buffer, which after each call
 *     holds that call's counts.  Any other overlap of the two is invalid.
 *   - Size: with counts of other data an archive can exceed dgpu_float_max_compressed_size (worst case probBits bits
 *     per symbol).  Nothing is stored beyond dgpu_float_max_compressed_size(floatType, inSize[i]) bytes of out[i], and
 *     outSize_dev[i] reports the FULL size: a value above that maximum means the archive is incomplete, and the caller
 *     compresses that call again with countsIn_dev = NULL.  The maximum allows 5120 bytes per 4096-word block plus the
 *     header of a 4096-block archive; a table that covers nothing costs about 623 bytes per block more at probBits 11,
 *     so this can happen from about 894 blocks (3.66 M words) at probBits 11 and from about 4900 blocks at probBits
 *     10, never below; tables of data whose distribution merely drifted are nowhere near it.
 *   - floatType is the type of the ARCHIVE, DGPU_FLOAT16 or DGPU_BFLOAT16 (float32 archives are out of scope: the
 *     float32 encoder has no counting form); sourceFloat32 0: in[i] holds floatType words, 2-byte aligned; 1: float32
 *     words, 4-byte aligned, rounded as by dgpu_float_cast_compress.  probBits 9 / 10 / 11, numInBatch <= 65535,
 *     out[i] 16-byte aligned, inSize[i] within the size guard of dgpu_float_compress: DGPU_ERR_INVALID_ARGUMENT
 *     otherwise, with a dgpu_last_error() text, before anything is enqueued.  An empty batch returns 0, *tempUsed = 0.
 *   - Temp memory: at most dgpu_float_compress_temp_bytes(floatType, numInBatch, max inSize).  Nothing synchronises;
 *     the call can be captured into a HIP graph after one identical warm call.  Stride detection, parameter cache and
 *     work lists are the plain call's; with countsIn_dev the batch is not split into size classes (as with a caller's
 *     histogram). */
int dgpu_float_rolling_compress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed,
    uint32_t floatType /* of the ARCHIVE: DGPU_FLOAT16 or DGPU_BFLOAT16 */,
    uint32_t sourceFloat32 /* 0: in[i] holds floatType words; 1: float32 words */,
    int probBits, uint32_t numInBatch, const void* const* in, const uint32_t* inSize /* words */,
    const uint32_t* countsIn_dev /* [numInBatch][256], nullable */,
    uint32_t* countsOut_dev /* [numInBatch][256], nullable */,
    void* const* out, uint32_t* outSize_dev, void* stream);

/* ---- reduce-compress (no upstream equivalent) ------------------------------------------
 * dgpu_float_decode_reduce into the float32 accumulators and dgpu_float_cast_compress of those accumulators in ONE
 * call: the middle of a compressed all-reduce, where the reduced shard is sent on at once.  The reduce kernel counts
 * the exponent bytes of the rounded sums while it stores them, so the cast histogram pass -- a second read of the shard --
 * does not run; the table is normalised from those counts and the cast encoder reads the accumulators once.
 *   - Accumulators: acc[i], outSuccess_dev[i] and outSize_dev[i] are bit for bit what dgpu_float_decode_reduce leaves
 *     for the same arguments (layout, order of the adds, widening, all-or-nothing, what outSize_dev reports), with ONE
 *     exception: every source of member i must state EXACTLY outCapacity[i] words -- the compress side codes
 *     outCapacity[i] words of the accumulator.  A member whose sources state fewer fails like any other failing member.
 *   - Archives, successful member: outArchive[i] and outArchiveSize_dev[i] (bytes) are byte for byte what
 *     dgpu_float_cast_compress(floatType, probBits) writes for acc[i] afterwards (rounding: see there).
 *   - Archives, failed member (outSuccess_dev[i] = 0): the accumulator keeps every bit; outArchive[i] is a well-formed
 *     archive of the cast of whatever the accumulator holds, coded with the flat table (every symbol the same
 *     probability): inside dgpu_float_max_compressed_size(floatType, outCapacity[i]) and decodable.  Look at
 *     outSuccess_dev before sending it on.
 *   - floatType is that of the sources AND of the archives: DGPU_FLOAT16 or DGPU_BFLOAT16.  DGPU_FLOAT32 is invalid
 *     (there is no cast to do: dgpu_float_decode_reduce, then dgpu_float_compress).
 *   - 1 <= numSources <= 64 (numSources == 1 does not forward anywhere: it is this call), numInBatch * numSources <=
 *     65535, accumulate 0 or 1, probBits 9, 10 or 11, in[...] and outArchive[i] 16-byte aligned, acc[i] 4-byte aligned,
 *     outCapacity[i] (words) within the size guard of dgpu_float_compress, no array null when numInBatch > 0
 *     (outSuccess_dev, outSize_dev and outArchiveSize_dev may be null): DGPU_ERR_INVALID_ARGUMENT otherwise, with a
 *     dgpu_last_error() text, before anything is enqueued.  An empty batch returns 0 with *tempUsed = 0.
 *   - outArchive[i] has room for dgpu_float_max_compressed_size(floatType, outCapacity[i]).  The accumulators of
 *     different members MUST NOT overlap each other or any archive buffer; sources may alias each other.
 *   - No useChecksum, for the reason its two halves have none.
 *   - Temp memory: at most dgpu_float_reduce_compress_temp_bytes(floatType, numInBatch, max outCapacity); too little
 *     behaves as in every other call (library-owned overflow memory).  The counts live in library-owned per-stream
 *     counters for numInBatch <= 64 and in temp memory beyond.  Nothing synchronises; capturable into a HIP graph after
 *     one identical warm call on the stream. */
size_t dgpu_float_reduce_compress_temp_bytes(uint32_t floatType, uint32_t numInBatch, uint32_t maxWords);
int dgpu_float_reduce_compress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources,
    const void* const* in /* [numInBatch * numSources] */, const uint32_t* inBytes /* same shape */,
    void* const* acc /* float32, [numInBatch] */, const uint32_t* outCapacity /* float words */,
    void* const* outArchive /* [numInBatch] */,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev /* words */, uint32_t* outArchiveSize_dev /* bytes */,
    void* stream);

/* ---- mixed sources: archives and raw rows (no upstream equivalent) ------------------------
 * dgpu_float_decode_reduce and dgpu_float_reduce_compress whose sources may be UNCOMPRESSED: the shard a rank already
 * holds takes its place in the rank-ordered sum without being compressed and decoded again.  Everything said of the two
 * calls above holds (layout, order of the adds, widening, all or nothing per member, what outSize_dev reports, temp
 * memory, no synchronisation, graph capture after one identical warm call), with these additions:
 *   - sourceKind: a HOST array of numInBatch * numSources bytes, member-major like `in`: 0, source k is an archive;
 *     1, it is RAW: in[k] points at inBytes[k] / wordBytes words of floatType (2 bytes for float16 and bfloat16, 4 for
 *     float32), aligned to the word size -- a shard row of a flat tensor is not 16-byte aligned in general; the kernel
 *     loads 16 bytes at a time from a 16-byte aligned row and 4 or 2 bytes at a time otherwise.
 *   - The count a raw source states is inBytes[k] / wordBytes.  It takes part in "all sources state the same word
 *     count" and in "<= outCapacity[i]" ("== outCapacity[i]" in reduce-compress) exactly like a header's; if source 0
 *     is raw, outSize_dev[i] is that count.  A member with a raw source whose count disagrees fails like any other.
 *   - The words are widened as decoded words are and added with one __fadd_rn in their place in source order: the
 *     result is bit for bit what the plain call leaves when every raw row is replaced by its archive.
 *   - All sources of a member raw is valid (no probability table is read for it), and so is numSources == 1 with a raw
 *     source, which stores or adds the widened row.
 *   - Raw sources MUST NOT overlap any accumulator or output archive of the call; they may alias each other and
 *     archive sources.
 *   - DGPU_ERR_INVALID_ARGUMENT, with a dgpu_last_error() text and before anything is enqueued, also for: sourceKind
 *     null with numInBatch > 0, a kind other than 0 or 1, a raw in[k] not aligned to the word size, a raw inBytes[k]
 *     that is not a multiple of it.  The 16-byte alignment is required of archive sources only.
 *   - sourceKind is part of the batch's description: it is in the resident parameter block and its cache key, so a
 *     call that differs from a warm one only in its kinds is a different batch (and, under capture, not a warm one).
 *   - With every kind 0 the calls ARE dgpu_float_decode_reduce / dgpu_float_reduce_compress: same kernels, same block. */
int dgpu_float_decode_reduce_mixed(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources,
    const void* const* in /* [numInBatch * numSources] */, const uint32_t* inBytes /* same shape */,
    const uint8_t* sourceKind /* HOST, same shape: 0 archive, 1 raw */,
    void* const* out /* float32, [numInBatch] */, const uint32_t* outCapacity /* float words, [numInBatch] */,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream);
int dgpu_float_reduce_compress_mixed(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources,
    const void* const* in /* [numInBatch * numSources] */, const uint32_t* inBytes /* same shape */,
    const uint8_t* sourceKind /* HOST, same shape: 0 archive, 1 raw */,
    void* const* acc /* float32, [numInBatch] */, const uint32_t* outCapacity /* float words */,
    void* const* outArchive /* [numInBatch] */,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev /* words */, uint32_t* outArchiveSize_dev /* bytes */,
    void* stream);

/* ---- scaled: the mean, or an unscaled sum, in the reduce kernel (no upstream equivalent) --
 * dgpu_float_decode_reduce_mixed and dgpu_float_reduce_compress_mixed with one float32 factor per call.  Every successful
 * member is left with
 *     acc[i] = fl32( U[i] * scale )
 * where U[i] is, bit for bit, what the unscaled call would have left: ((acc + x0) + x1) + ... with accumulate,
 * (x0 + x1) + ... without, the widened source for numSources == 1 without.  The product is one IEEE float32 multiply
 * (__fmul_rn: round to nearest even, denormals kept, never contracted), made where the sum is in registers, on the last
 * source's store: no pass over the data, no second rounding, and an overflow of the SUM's rounding to the archive type
 * cannot happen to a mean that is representable.  With accumulate == 1 the factor covers the old accumulator contents too.
 *   - Reduce-compress rounds and counts the SCALED value: a successful member's archive is byte for byte what
 *     dgpu_float_cast_compress writes for the scaled accumulator.  The encoder is untouched.
 *   - Everything else is the contract of the mixed calls: order of the adds, all or nothing per member, outSuccess_dev and
 *     outSize_dev, a failed member keeps every bit of its accumulator (and gets a decodable flat-table archive), raw
 *     rows, capacities, temp memory (reduce-compress: within dgpu_float_reduce_compress_temp_bytes), no host
 *     synchronisation, graph capture after one identical warm call.
 *   - sourceKind may be NULL: every source is an archive.
 *   - scale must be finite and not zero: otherwise DGPU_ERR_INVALID_ARGUMENT, with a dgpu_last_error() text, before
 *     anything is enqueued.
 *   - scale == 1.0f IS the unscaled call (the mixed one, or with sourceKind NULL the plain one): same kernels, same
 *     parameter block, no multiply -- a signalling NaN stored by numSources == 1, accumulate == 0 keeps its bits.
 *   - With any other scale numSources == 1 runs the reducing kernel as well (decode-reduce does not forward to
 *     decode-accumulate, which does not scale).
 *   - The scale is a kernel argument and not part of the resident parameter block: calls that differ only in it share
 *     the block and its cache entry.  A captured call has its scale baked in. */
int dgpu_float_decode_reduce_scaled(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources,
    const void* const* in /* [numInBatch * numSources] */, const uint32_t* inBytes /* same shape */,
    const uint8_t* sourceKind /* HOST, same shape: 0 archive, 1 raw; NULL: all archives */, float scale,
    void* const* out /* float32, [numInBatch] */, const uint32_t* outCapacity /* float words, [numInBatch] */,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream);
int dgpu_float_reduce_compress_scaled(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources,
    const void* const* in /* [numInBatch * numSources] */, const uint32_t* inBytes /* same shape */,
    const uint8_t* sourceKind /* HOST, same shape: 0 archive, 1 raw; NULL: all archives */, float scale,
    void* const* acc /* float32, [numInBatch] */, const uint32_t* outCapacity /* float words */,
    void* const* outArchive /* [numInBatch] */,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev /* words */, uint32_t* outArchiveSize_dev /* bytes */,
    void* stream);

/* ---- norm: the squared norm and the non-finite count of what a reduce call leaves (no upstream equivalent) --
 * dgpu_float_decode_reduce_scaled and dgpu_float_reduce_compress_scaled with two more outputs per member, for gradient
 * clipping by global norm and for the overflow check of loss scaling, which otherwise read the reduced shard again:
 *     outSumSq_dev[i]     float64: the sum of w * w over the FINITE measured words w of member i, each w widened exactly
 *     outNonFinite_dev[i] uint32:  the number of measured words that are +-inf or NaN
 *   - The measured words.  Decode-reduce: the float32 words the call leaves in out[i] -- after the last add, after the
 *     multiply by scale, with accumulate == 1 including the old contents; exactly as many as the member's sources state
 *     (a prefix of a larger capacity is measured as a prefix).  Reduce-compress: the words of the ARCHIVE -- those float32
 *     words rounded to floatType by the cast encoder's own rounding, the tensor every rank holds after the all-gather.  A
 *     float32 sum of 70000 is finite and its float16 rounding is not: reduce-compress counts it non-finite.
 *   - Precision: the square of a float32 is exact in float64 and the squares are added in float64, so the result lies
 *     within relative n * 2^-52 of the exact sum over the n measured words, and squares beyond the float32 range stay
 *     finite.
 *   - A member with outSuccess_dev[i] == 0, and an empty member, gets 0.0 and 0.
 *   - Determinism: the same call with the same arguments and library settings leaves the same 64 bits every time,
 *     whatever the order the workgroups run in (work lists, decoder order): a tile's words are added in a fixed order,
 *     the tiles of a member in tile order, without floating-point atomics.  Bit equality is NOT promised between calls
 *     that differ in tile geometry (the largest capacity of the batch) or in probBits; the bound holds for all.
 *   - Everything else the call leaves -- accumulators, outSuccess_dev, outSize_dev, archives, archive sizes -- is bit for
 *     bit what the scaled call with the same arguments leaves.
 *   - scale as in the scaled calls; here 1.0f multiplies nothing either (a signalling NaN keeps its bits).  sourceKind
 *     may be NULL: every source is an archive.
 *   - Either output pointer may be NULL and is then not written; with both NULL the call IS the scaled call.
 *     outSumSq_dev must be 8-byte aligned, outNonFinite_dev 4-byte aligned: otherwise DGPU_ERR_INVALID_ARGUMENT with a
 *     dgpu_last_error() text, like every argument error before anything is enqueued.
 *   - Temp memory: one float64 and one uint32 per member and tile, at most
 *     dgpu_float_reduce_norm_temp_bytes(floatType, numInBatch, max outCapacity, compress) with compress != 0 for
 *     reduce-compress (whose own temp memory it includes); *tempUsed reports it; too little falls back to library-owned
 *     overflow memory.  These are the only decode-side calls that use temp memory.
 *   - No host synchronisation; capturable into a HIP graph after one identical warm call. */
size_t dgpu_float_reduce_norm_temp_bytes(uint32_t floatType, uint32_t numInBatch, uint32_t maxWords, int compress);
int dgpu_float_decode_reduce_norm(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources,
    const void* const* in /* [numInBatch * numSources] */, const uint32_t* inBytes /* same shape */,
    const uint8_t* sourceKind /* HOST, same shape: 0 archive, 1 raw; NULL: all archives */, float scale,
    void* const* out /* float32, [numInBatch] */, const uint32_t* outCapacity /* float words, [numInBatch] */,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev,
    double* outSumSq_dev /* [numInBatch], nullable */, uint32_t* outNonFinite_dev /* [numInBatch], nullable */, void* stream);
int dgpu_float_reduce_compress_norm(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources,
    const void* const* in /* [numInBatch * numSources] */, const uint32_t* inBytes /* same shape */,
    const uint8_t* sourceKind /* HOST, same shape: 0 archive, 1 raw; NULL: all archives */, float scale,
    void* const* acc /* float32, [numInBatch] */, const uint32_t* outCapacity /* float words */,
    void* const* outArchive /* [numInBatch] */,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev /* words */, uint32_t* outArchiveSize_dev /* bytes */,
    double* outSumSq_dev /* [numInBatch], nullable */, uint32_t* outNonFinite_dev /* [numInBatch], nullable */, void* stream);

/* ---- float stride batches with capacities (no upstream equivalent) ---------------
 * For exchanging compressed rows at a FIXED width (README.md:68-72,104: compressed collectives): the rows of one
 * tensor are compressed straight into the rows of the send matrix, `outStrideBytes` apart, and nothing is stored
 * beyond `outCapacityBytes` of a row -- a row whose archive is longer (outSize_dev[i] > outCapacityBytes) is
 * incomplete and must be sent another way; outSize_dev reports the full size either way.  The capacity must hold
 * everything but the block data (header, tables, non-compressed planes: DGPU_ERR_INVALID_ARGUMENT otherwise), rows
 * have more than 4096 words.  The receiving side decodes rows of `inBytes` available bytes each; a row whose
 * archive claims more is reported through outSuccess_dev and not read (as the *_bounded entry points above). */
int dgpu_float_compress_stride_capped(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch, const void* in_dev, uint32_t inWords, uint32_t inStrideBytes,
    void* out_dev, uint32_t outStrideBytes, uint32_t outCapacityBytes, uint32_t* outSize_dev, void* stream);
int dgpu_float_decompress_stride_bounded(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch, const void* in_dev, uint32_t inStrideBytes, uint32_t inBytes,
    void* out_dev, uint32_t outStrideBytes, uint32_t outCapacityWords,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream, int32_t* errBatch);

/* floatGetCompressedInfo, GpuFloatCodec.h:264-277 / GpuFloatInfo.cu:17-45 */
int dgpu_float_get_compressed_info(
    void* temp_dev, size_t tempBytes,
    const void* const* in, uint32_t numInBatch,
    uint32_t* outSizes_dev, uint32_t* outTypes_dev, uint32_t* outChecksum_dev,
    void* stream);
/* floatGetCompressedInfoDevice, GpuFloatCodec.h:279-292 / GpuFloatInfo.cu:47-64 */
int dgpu_float_get_compressed_info_device(
    const void* const* in_dev, uint32_t numInBatch,
    uint32_t* outSizes_dev, uint32_t* outTypes_dev, uint32_t* outChecksum_dev,
    void* stream);

/* ---- building blocks exposed for parity tests ----------------------------- */
/* ansHistogramBatch, GpuANSStatistics.cuh:384-412: [B][256] u32 counts of a
 * strided batch (any byte alignment). */
int dgpu_ans_histogram_batch_stride(
    uint32_t numInBatch,
    const void* in_dev, uint32_t inPerBatchSize, uint32_t inPerBatchStride,
    uint32_t* histogram_dev,
    void* stream);
/* ansCalcWeights, GpuANSStatistics.cuh:414-430: normalised {pdf,cdf,magic,shift}
 * uint4[B][256] in the REFERENCE's table layout (the encoder itself uses a
 * re-packed table). */
int dgpu_ans_calc_weights(
    uint32_t numInBatch, int probBits,
    const uint32_t* sizes_dev, uint32_t uniformSize,
    const uint32_t* histogram_dev,
    uint32_t* table_dev,
    void* stream);

/* ---- library-owned device state (no upstream equivalent) -------------------- */
/* The library keeps a little device memory per (device, stream) it has been used
 * on: the temp-memory overflow slab (what StackDeviceMemory.cpp:119-139 would
 * cudaMalloc/cudaFree per call) and the zero-at-rest hand-off counters of the
 * histogram pass.  It is bounded (the least recently used idle states are dropped
 * beyond 32 streams), and can be given back explicitly: synchronises the device,
 * frees the memory kept for `stream` on the current device (or for every stream),
 * returns the number of states released.  Call before destroying a stream. */
int dgpu_release_stream_state(void* stream);
int dgpu_release_all_stream_state(void);
/* Test hook: number of (device, stream) states currently kept. */
uint32_t dgpu_debug_stream_state_count(void);
/* Test hook: synchronises `stream`, copies the hand-off counters the library keeps for it on the current device to the
 * host -- 65536 arrival words, 64 x 256 histogram counters, 16384 spill-pool flags, all zero at rest -- and returns how
 * many of them are not zero; -1 when the stream has no state or no counters yet (asking creates none), or is being
 * captured. */
int64_t dgpu_debug_counters_nonzero(void* stream);

/* ---- instrumentation (no upstream equivalent) ------------------------------ */
/* Per-kernel timing with HIP events recorded on the launch stream; used by
 * bench.py for the roofline figure.  Off by default. */
void dgpu_prof_enable(int on);
void dgpu_prof_reset(void);
/* Writes a JSON object {"kernel": {"launches": n, "total_ms": t}, ...} into buf
 * (synchronises on the recorded events). Returns length, or -1 if cap is too small. */
int dgpu_prof_summary(char* buf, size_t cap);

/* Test hook: makes every encoder workgroup whose index is congruent to 1 modulo
 * `modulo` start about half a millisecond after the others (0 = off, the
 * default).  It emulates a grid that is only partly resident at first -- other
 * kernels holding compute units -- so that tests can exercise the path in which
 * running workgroups take over the tiles of workgroups that have not started. */
void dgpu_debug_set_absent_workgroups(uint32_t modulo);

/* Measurement / test hook: how the workgroups of the tiled encoder (k_ans_encode; replaces the grid of ansEncodeBatch,
 * GpuANSEncode.cuh:429-461) come to their tiles -- for raw bytes and for float tiles of 2 or 4 blocks, the kernels that
 * exist in both forms.  -1 (default): the library decides per call (one workgroup per tile when there are more tiles
 * than resident workgroups); 0: as many persistent workgroups as fit on the device, static ticket map; 1: one workgroup
 * per tile, dispatched by the hardware in ticket order.  Archives are byte-identical either way.  8-block float tiles
 * always run persistent, single-block elements always one workgroup per pair. */
void dgpu_debug_set_encoder_dispatch(int mode);

/* Measurement / test hook: the order in which the workgroups of the tiled decoder (k_ans_decode; replaces the grid of
 * ansDecodeBatch, GpuANSDecode.cuh:299-403) take the (element, tile) pairs.  -1 (default): the library decides per
 * call; 0: element-major; 1: tile-major; 2: every XCD walks its own elements.  Outputs are identical either way. */
void dgpu_debug_set_decoder_order(int order);

/* Measurement / test hook: batches whose elements differ widely in size (the tensors of a model in one call).  The
 * grids of upstream's kernels -- and this library's -- are rectangles laid out for the largest element
 * (GpuANSEncode.cuh:692-760, GpuANSDecode.cuh:299-403: maxSize x numInBatch); here the sizes arrive as host arrays, so
 * for a batch in which at least a fifth of that rectangle would be empty the host lists the tiles and histogram parts
 * that exist and the kernels work through the lists.  -1 (default): that policy; 0: always the rectangles; 1: the
 * lists for every pointer-array call whose sizes differ.  Archives and outputs are byte-identical either way.  The
 * ranged decode calls are not affected: they have no rectangle and always list the tiles of their ranges. */
void dgpu_debug_set_work_lists(int mode);

/* Measurement / test hook: SIZE CLASSES inside one batch.  Upstream sizes the one grid of a call for its largest member
 * (GpuANSEncode.cuh:753-771, GpuANSDecode.cuh:299-403); here a pointer-array call whose members fall into more than one
 * of the classes {one block, <= 2, <= 4 (decode: <= 8), more} launches every class on the kernels of its own geometry,
 * one class after the other on the caller's stream.  -1 (default): when the smaller classes together hold at least 256
 * members, classes of fewer than 32 joining the next larger one; 0: one geometry per call; 1: every class that has a
 * member.  Needs the work lists (dgpu_debug_set_work_lists != 0).  Archives and outputs are byte-identical either way. */
void dgpu_debug_set_size_classes(int mode);

/* Measurement hook: 0 makes every pointer-array call upload its parameter block
 * (no reuse of blocks already resident on the device); 1 (default) restores the
 * cache.  bench.py uses it to report the step time without the cache next to the
 * steady-state one. */
void dgpu_debug_set_param_cache(int on);

/* Cache policy of the encoder's histogram pass (its first kernel; the second reads the same input again): 0 = the
 * input is read with non-temporal loads (default), 1 = with ordinary loads, which allocate in the 256 MiB memory-side
 * cache -- the pass then also pays for evicting whatever dirty lines sit there and the encode kernel reads its input
 * from the cache.  Worth ~9 % where the codec's own output is what fills the cache (compress followed at once by
 * decompress on the same device, on buffers that change every call), a loss of 4-20 % otherwise (DESIGN.md
 * section 5).  -1 restores the default.  Process-wide; archives are identical either way. */
void dgpu_set_histogram_load_policy(int mode);

/* HIP graphs.  A call made while its stream is being captured (hipStreamBeginCapture) bakes library-owned device
 * addresses into the graph: the resident copy of its pointer / size arrays and the stream's hand-off counters and
 * overflow slab.  The library pins them -- they are neither evicted nor trimmed nor released by
 * dgpu_release_stream_state / dgpu_release_all_stream_state -- until the caller, having destroyed every such graph,
 * calls dgpu_release_graph_state() (returns the number of objects unpinned / released; synchronises the devices).
 * Nothing can be uploaded or allocated under capture: a call whose arrays are not resident yet, or whose temp
 * memory overflows into a slab that would have to grow, fails with DGPU_ERR_HIP and a message that says so; running
 * the same call once before capturing makes everything resident. */
int dgpu_release_graph_state(void);

#ifdef __cplusplus
}
#endif
#endif /* DIETGPU_AMD_H */
