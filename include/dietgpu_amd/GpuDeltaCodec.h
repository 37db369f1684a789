// XOR-delta archives in the style of the dietgpu:: mirror (no reference equivalent): a tensor coded against a near copy
// of it that the receiver already holds.  ansEncodeBatchDelta writes, for every element, the ordinary raw-byte ANS archive
// of in[i] ^ base[i] -- byte for byte what ansEncodeBatchPointer writes for the XOR-ed bytes, without a checksum -- and
// ansDecodeBatchDelta leaves out[i] = decoded ^ base[i], where out[i] may BE base[i]: in place, the base becomes the new
// tensor, and a member that fails keeps every byte of it.  Both XOR in the codec's own kernels: no scratch tensor, no
// extra pass.  Inline on top of dgpu_ans_delta_encode / dgpu_ans_delta_decode of ../dietgpu_amd.h, where the contract is
// spelled out.  `inSize`, `inBytes`, `outCapacity`: bytes.  The config's useChecksum is ignored.  Neither call takes temp
// memory -- their temporaries are the stream's own: there is no StackDeviceMemory parameter.
#pragma once

#include "GpuANSCodec.h"

namespace dietgpu {

inline void ansEncodeBatchDelta(
    const ANSCodecConfig& config, uint32_t numInBatch, const void** in, const void** base, const uint32_t* inSize, void** out,
    uint32_t* outSize_dev, hipStream_t stream) {
  detail::checkRc(dgpu_ans_delta_encode(config.probBits, numInBatch, in, base, inSize, out, outSize_dev, stream), "ansEncodeBatchDelta");
}

inline void ansDecodeBatchDelta(
    const ANSCodecConfig& config, uint32_t numInBatch, const void** in, const uint32_t* inBytes, const void** base, void** out,
    const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  detail::checkRc(dgpu_ans_delta_decode(config.probBits, numInBatch, in, inBytes, base, out, outCapacity, outSuccess_dev, outSize_dev, stream),
                  "ansDecodeBatchDelta");
}

}  // namespace dietgpu
