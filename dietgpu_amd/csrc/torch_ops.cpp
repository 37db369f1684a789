// torch.ops.dietgpu.* on PyTorch-ROCm: the ten ops of dietgpu/DietGpu.cpp with
// the schema strings kept verbatim (DietGpu.cpp:915-937), implemented on top of
// the C ABI of include/dietgpu_amd.h.  Host-only C++ (no kernels here); tensors
// are plumbing for device memory and the current HIP stream.
//
// Same argument validation and error behaviour as the reference
// (TORCH_CHECK -> c10::Error): DietGpu.cpp:149-275 (compress_data_res),
// :310-452 (split size), :454-522 (simple), :530-644 (decompress_data_res),
// :679-816, :818-911.
#include <ATen/ATen.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cmath>
#include <optional>
#include <tuple>
#include <vector>

#include "../../include/dietgpu_amd.h"

namespace dietgpu_amd {
namespace {

constexpr int kDefaultPrecision = 10;  // DietGpu.cpp:114
// The precision the six codec ops use on the calling thread.  The reference's ops fix it at kDefaultPrecision; its C++
// API takes it per call (ANSCodecConfig.probBits, GpuANSCodec.h:28-51).  dietgpu_amd::set_precision (an EXTRA op, in
// its own namespace) lets dietgpu_amd.ops serve `prob_bits` 9 / 11 through this library too instead of through ctypes.
thread_local int tPrecision = kDefaultPrecision;
int precision() { return tPrecision; }

uint32_t floatTypeFromDtype(at::ScalarType t) {
  switch (t) {
    case at::ScalarType::Half: return DGPU_FLOAT16;
    case at::ScalarType::BFloat16: return DGPU_BFLOAT16;
    case at::ScalarType::Float: return DGPU_FLOAT32;
    default:
      TORCH_CHECK(false, "dietgpu: tensor must be float16, bfloat16 or float32");
  }
  return DGPU_FLOAT_UNDEFINED;
}

at::ScalarType dtypeFromFloatType(uint32_t ft) {
  switch (ft) {
    case DGPU_FLOAT16: return at::ScalarType::Half;
    case DGPU_BFLOAT16: return at::ScalarType::BFloat16;
    case DGPU_FLOAT32: return at::ScalarType::Float;
    default:
      TORCH_CHECK(false, "dietgpu: unknown float type in archive");
  }
  return at::ScalarType::Half;
}

std::tuple<int64_t, int64_t> totalAndMaxSize(const std::vector<at::Tensor>& ts) {
  int64_t total = 0, mx = 0;
  for (auto& t : ts) {
    auto n = t.numel();
    TORCH_CHECK((uint64_t)(n * t.element_size()) <= std::numeric_limits<uint32_t>::max());
    total += n;
    mx = std::max<int64_t>(mx, n);
  }
  return {total, mx};
}

// the size queries return 0 beyond the reference's INT32_MAX guard (getMaxCompressedSize's CHECK_LE, GpuANSEncode.cu:22)
uint32_t maxAnsSize(uint64_t bytes) {
  TORCH_CHECK(bytes <= 0xffffffffull, "input of ", bytes, " bytes: sizes are 32-bit (GpuANSCodec.h)");
  const uint32_t r = dgpu_ans_max_compressed_size((uint32_t)bytes);
  TORCH_CHECK(r != 0, "input of ", bytes, " bytes: its maximum compressed size exceeds INT32_MAX (GpuANSEncode.cu:22)");
  return r;
}
uint32_t maxFloatSize(uint32_t ft, uint64_t words) {
  TORCH_CHECK(words <= 0xffffffffull, "tensor of ", words, " words: sizes are 32-bit (GpuFloatCodec.h)");
  const uint32_t r = dgpu_float_max_compressed_size(ft, (uint32_t)words);
  TORCH_CHECK(r != 0, "tensor of ", words, " words: the maximum compressed size exceeds INT32_MAX (GpuANSEncode.cu:22)");
  return r;
}

void* streamOf(int dev) { return (void*)c10::hip::getCurrentHIPStream(dev).stream(); }

void check(int rc, const char* what, bool isFloat) {
  // (DietGpu.cpp:626-633 / 801-808 raise this text; the members are what upstream's errorInfo lists)
  TORCH_CHECK(rc != DGPU_ERR_CHECKSUM_MISMATCH, isFloat ? "floatDecompress" : "ANSDecode",
              ": checksum mismatch seen on decoded data; archive cannot be unpacked\n", dgpu_last_error());
  TORCH_CHECK(rc == DGPU_OK, what, " failed: ", dgpu_last_error());
}

struct Temp {
  void* ptr = nullptr;
  size_t bytes = 0;
};
Temp tempOf(const std::optional<at::Tensor>& t, int dev) {
  Temp r;
  if (t) {
    TORCH_CHECK(t->device().is_cuda());
    TORCH_CHECK(t->is_contiguous());
    TORCH_CHECK(t->get_device() == dev);
    r.ptr = t->data_ptr();
    r.bytes = (size_t)t->numel() * t->element_size();
  }
  return r;
}

void validateCompOut(
    const std::optional<at::Tensor>& outCompressed, const std::optional<at::Tensor>& outSizes,
    int64_t rows, int64_t cols, int dev, const at::Device& device, at::Tensor& comp, at::Tensor& sizes) {
  if (outCompressed) {
    TORCH_CHECK(outCompressed->dtype() == at::kByte);
    TORCH_CHECK(outCompressed->device().is_cuda());
    TORCH_CHECK(outCompressed->is_contiguous());
    TORCH_CHECK(outCompressed->dim() == 2);
    TORCH_CHECK(outCompressed->size(0) >= rows);
    TORCH_CHECK(outCompressed->size(1) >= cols);
    TORCH_CHECK(outCompressed->get_device() == dev);
    comp = *outCompressed;
  } else {
    comp = at::empty({rows, cols}, at::TensorOptions().device(device).dtype(at::kByte));
  }
  if (outSizes) {
    TORCH_CHECK(outSizes->dtype() == at::kInt);
    TORCH_CHECK(outSizes->device().is_cuda());
    TORCH_CHECK(outSizes->dim() == 1);
    TORCH_CHECK(outSizes->is_contiguous());
    TORCH_CHECK(outSizes->size(0) >= rows);
    TORCH_CHECK(outSizes->get_device() == dev);
    sizes = *outSizes;
  } else {
    sizes = at::empty({rows}, at::TensorOptions().device(device).dtype(at::kInt));
  }
}

void validateStatus(const std::optional<at::Tensor>& outStatus, const std::optional<at::Tensor>& outSizes, int64_t n, int dev) {
  if (outStatus) {
    TORCH_CHECK(outStatus->is_contiguous());
    TORCH_CHECK(outStatus->device().is_cuda());
    TORCH_CHECK(outStatus->dtype() == at::kByte);
    TORCH_CHECK(outStatus->numel() == n);
    TORCH_CHECK(outStatus->get_device() == dev);
  }
  if (outSizes) {
    TORCH_CHECK(outSizes->is_contiguous());
    TORCH_CHECK(outSizes->device().is_cuda());
    TORCH_CHECK(outSizes->dtype() == at::kInt);
    TORCH_CHECK(outSizes->numel() == n);
    TORCH_CHECK(outSizes->get_device() == dev);
  }
}

template <typename T>
T* ptrOrNull(const std::optional<at::Tensor>& t) { return t ? (T*)t->data_ptr() : nullptr; }

// The tensor pairs of a decode call as the C ABI takes them: the checks of each pair (`extra(i)`: the caller's own, made
// between them and the marshalling) and the four arrays.
struct DecodeTensors {
  std::vector<const void*> inPtrs;
  std::vector<void*> outPtrs;
  std::vector<uint32_t> outCapacity;
  std::vector<uint32_t> inBytes;  // the tensors say how many bytes each archive may occupy
};
template <typename Extra>
DecodeTensors marshalDecode(bool compressAsFloat, const std::vector<at::Tensor>& tIns, const std::vector<at::Tensor>& tOuts, int dev, Extra extra) {
  const size_t n = tIns.size();
  DecodeTensors m{std::vector<const void*>(n), std::vector<void*>(n), std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
  for (size_t i = 0; i < n; ++i) {
    auto& tIn = tIns[i];
    auto& tOut = tOuts[i];
    TORCH_CHECK(tIn.device().is_cuda());
    TORCH_CHECK(tIn.get_device() == dev);
    TORCH_CHECK(tIn.is_contiguous());
    TORCH_CHECK(tOut.device().is_cuda());
    TORCH_CHECK(tOut.get_device() == dev);
    TORCH_CHECK(tOut.is_contiguous());
    TORCH_CHECK(tIn.dtype() == at::kByte);
    if (compressAsFloat) floatTypeFromDtype(tOut.scalar_type());
    extra(i);
    m.inPtrs[i] = tIn.data_ptr();
    m.inBytes[i] = (uint32_t)std::min<int64_t>(tIn.numel(), std::numeric_limits<uint32_t>::max());
    m.outPtrs[i] = tOut.data_ptr();
    auto cap = compressAsFloat ? tOut.numel() : tOut.numel() * tOut.element_size();
    TORCH_CHECK((uint64_t)cap <= std::numeric_limits<uint32_t>::max());
    m.outCapacity[i] = (uint32_t)cap;
  }
  return m;
}

}  // namespace

// ---- size queries (DietGpu.cpp:116-143) --------------------------------------
std::tuple<int64_t, int64_t> max_float_compressed_output_size(const std::vector<at::Tensor>& ts) {
  TORCH_CHECK(!ts.empty());
  auto sz = totalAndMaxSize(ts);
  return {(int64_t)ts.size(),
          (int64_t)maxFloatSize(floatTypeFromDtype(ts[0].scalar_type()), (uint64_t)std::get<1>(sz))};
}

int64_t max_float_compressed_size(const at::Tensor& dtype, int64_t size) {
  return maxFloatSize(floatTypeFromDtype(dtype.scalar_type()), (uint64_t)size);
}

std::tuple<int64_t, int64_t> max_any_compressed_output_size(const std::vector<at::Tensor>& ts) {
  TORCH_CHECK(!ts.empty());
  auto sz = totalAndMaxSize(ts);
  return {(int64_t)ts.size(), (int64_t)maxAnsSize((uint64_t)std::get<1>(sz) * ts[0].element_size())};
}

int64_t max_any_compressed_size(int64_t bytes) { return maxAnsSize((uint64_t)bytes); }

// ---- compress ------------------------------------------------------------------
std::tuple<at::Tensor, at::Tensor, int64_t> compress_data(
    bool compressAsFloat, const std::vector<at::Tensor>& tIns, bool checksum,
    const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& outCompressed,
    const std::optional<at::Tensor>& outCompressedSizes) {
  TORCH_CHECK(!tIns.empty());
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  Temp tmp = tempOf(tempMem, dev);

  auto maxOut = compressAsFloat ? max_float_compressed_output_size(tIns) : max_any_compressed_output_size(tIns);
  for (auto& t : tIns) {
    TORCH_CHECK(t.device().is_cuda());
    TORCH_CHECK(t.is_contiguous());
    TORCH_CHECK(t.get_device() == dev);
    if (compressAsFloat) {
      TORCH_CHECK(t.dtype() == tIns[0].dtype());
      floatTypeFromDtype(t.scalar_type());
    }
  }
  at::Tensor comp, sizes;
  validateCompOut(outCompressed, outCompressedSizes, (int64_t)tIns.size(), std::get<1>(maxOut), dev, tIns[0].device(), comp, sizes);

  const size_t n = tIns.size();
  std::vector<const void*> inPtrs(n);
  std::vector<uint32_t> inSize(n);
  std::vector<void*> compPtrs(n);
  for (size_t i = 0; i < n; ++i) {
    inPtrs[i] = tIns[i].data_ptr();
    inSize[i] = compressAsFloat ? tIns[i].numel() : tIns[i].numel() * tIns[i].element_size();
    compPtrs[i] = (uint8_t*)comp.data_ptr() + i * comp.size(1);
  }
  size_t used = 0;
  if (compressAsFloat) {
    check(dgpu_float_compress(tmp.ptr, tmp.bytes, &used, floatTypeFromDtype(tIns[0].scalar_type()), precision(),
                              checksum, (uint32_t)n, inPtrs.data(), inSize.data(), compPtrs.data(),
                              (uint32_t*)sizes.data_ptr(), streamOf(dev)),
          "floatCompress", true);
  } else {
    check(dgpu_ans_encode_batch_pointer(tmp.ptr, tmp.bytes, &used, precision(), checksum, (uint32_t)n,
                                        inPtrs.data(), inSize.data(), nullptr, compPtrs.data(),
                                        (uint32_t*)sizes.data_ptr(), streamOf(dev)),
          "ansEncodeBatchPointer", false);
  }
  return {std::move(comp), std::move(sizes), (int64_t)used};
}

std::tuple<std::vector<at::Tensor>, at::Tensor, int64_t> compress_data_split_size(
    bool compressAsFloat, const at::Tensor& tIn, const at::Tensor& tSplitSizes, bool checksum,
    const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& outCompressed,
    const std::optional<at::Tensor>& outCompressedSizes) {
  int dev = tIn.get_device();
  c10::hip::HIPGuard guard(dev);
  Temp tmp = tempOf(tempMem, dev);

  TORCH_CHECK(tIn.device().is_cuda());
  TORCH_CHECK(tIn.is_contiguous());
  uint32_t ft = compressAsFloat ? floatTypeFromDtype(tIn.scalar_type()) : DGPU_FLOAT_UNDEFINED;
  if (!compressAsFloat) {
    TORCH_CHECK(uintptr_t(tIn.data_ptr()) % DGPU_ANS_REQUIRED_ALIGNMENT == 0,
                "All splits should start on a 16 byte boundary; start pointer is not aligned");
  }
  auto numInBatch = tSplitSizes.numel();
  TORCH_CHECK(tSplitSizes.is_contiguous());
  TORCH_CHECK(tSplitSizes.device().is_cpu());
  TORCH_CHECK(tSplitSizes.dtype() == at::kInt);
  uint32_t maxSize = 0;
  for (int64_t i = 0; i < numInBatch; ++i) {
    auto size = ((const int32_t*)tSplitSizes.data_ptr())[i];
    TORCH_CHECK(size > 0);
    maxSize = std::max((uint32_t)size, maxSize);
    if (!compressAsFloat && i != numInBatch - 1) {
      TORCH_CHECK(size % DGPU_ANS_REQUIRED_ALIGNMENT == 0,
                  "All splits should start on a 16 byte boundary; the size of an interior split is not a multiple of 16 bytes");
    }
  }
  int64_t maxCompressedBytes = compressAsFloat ? maxFloatSize(ft, maxSize) : maxAnsSize(maxSize);
  at::Tensor comp, sizes;
  validateCompOut(outCompressed, outCompressedSizes, numInBatch, maxCompressedBytes, dev, tIn.device(), comp, sizes);

  size_t used = 0;
  if (compressAsFloat) {
    check(dgpu_float_compress_split_size(tmp.ptr, tmp.bytes, &used, ft, precision(), checksum, (uint32_t)numInBatch,
                                         tIn.data_ptr(), (const uint32_t*)tSplitSizes.data_ptr(), comp.data_ptr(),
                                         (uint32_t)comp.size(1), (uint32_t*)sizes.data_ptr(), streamOf(dev)),
          "floatCompressSplitSize", true);
  } else {
    check(dgpu_ans_encode_batch_split_size(tmp.ptr, tmp.bytes, &used, precision(), checksum, (uint32_t)numInBatch,
                                           tIn.data_ptr(), (const uint32_t*)tSplitSizes.data_ptr(), nullptr,
                                           comp.data_ptr(), (uint32_t)comp.size(1), (uint32_t*)sizes.data_ptr(),
                                           streamOf(dev)),
          "ansEncodeBatchSplitSize", false);
  }
  // compressedMatrixToTensors (DietGpu.cpp:77-104): views narrowed to the reported sizes
  at::Tensor sizesHost = sizes.to(at::kCPU);
  auto flat = comp.view({comp.numel()});
  std::vector<at::Tensor> out(numInBatch);
  for (int64_t i = 0; i < numInBatch; ++i) {
    out[i] = flat.narrow(0, i * comp.size(1), ((const int32_t*)sizesHost.data_ptr())[i]);
  }
  return {std::move(out), std::move(sizes), (int64_t)used};
}

std::vector<at::Tensor> compress_data_simple(
    bool compressAsFloat, const std::vector<at::Tensor>& tIns, bool checksum, const std::optional<int64_t>& tempMem) {
  TORCH_CHECK(!tIns.empty());
  std::optional<at::Tensor> scratch;
  if (tempMem && *tempMem > 0) {
    scratch = at::empty({*tempMem}, at::TensorOptions().device(tIns[0].device()).dtype(at::kByte));
  }
  auto comp = compress_data(compressAsFloat, tIns, checksum, scratch, std::nullopt, std::nullopt);
  auto& mat = std::get<0>(comp);
  at::Tensor sizeHost = std::get<1>(comp).to(at::kCPU);
  std::vector<at::Tensor> out;
  for (size_t i = 0; i < tIns.size(); ++i) {
    auto n = ((const int32_t*)sizeHost.data_ptr())[i];
    out.emplace_back(mat[i].narrow(0, 0, n).clone());
  }
  return out;
}

// ---- decompress ----------------------------------------------------------------
int64_t decompress_data_impl(
    bool compressAsFloat, const std::vector<at::Tensor>& tIns, const std::vector<at::Tensor>& tOuts, bool checksum,
    Temp tmp, const std::optional<at::Tensor>& outStatus, const std::optional<at::Tensor>& outSizes) {
  TORCH_CHECK(!tIns.empty());
  TORCH_CHECK(tIns.size() == tOuts.size());
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  const size_t n = tIns.size();
  DecodeTensors m = marshalDecode(compressAsFloat, tIns, tOuts, dev, [](size_t) {});
  validateStatus(outStatus, outSizes, (int64_t)n, dev);
  size_t used = 0;
  int32_t err = -1;
  if (compressAsFloat) {
    check(dgpu_float_decompress_bounded(tmp.ptr, tmp.bytes, &used, floatTypeFromDtype(tOuts[0].scalar_type()), precision(),
                                checksum, (uint32_t)n, m.inPtrs.data(), m.inBytes.data(), m.outPtrs.data(), m.outCapacity.data(),
                                ptrOrNull<uint8_t>(outStatus), ptrOrNull<uint32_t>(outSizes), streamOf(dev), &err),
          "floatDecompress", true);
  } else {
    check(dgpu_ans_decode_batch_pointer_bounded(tmp.ptr, tmp.bytes, &used, precision(), checksum, (uint32_t)n,
                                        m.inPtrs.data(), m.inBytes.data(), m.outPtrs.data(), m.outCapacity.data(),
                                        ptrOrNull<uint8_t>(outStatus), ptrOrNull<uint32_t>(outSizes), streamOf(dev), &err),
          "ansDecodeBatchPointer", false);
  }
  return (int64_t)used;
}

int64_t decompress_data(
    bool compressAsFloat, const std::vector<at::Tensor>& tIns, const std::vector<at::Tensor>& tOuts, bool checksum,
    const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& outStatus,
    const std::optional<at::Tensor>& outSizes) {
  TORCH_CHECK(!tIns.empty());
  int dev = tIns.front().get_device();
  return decompress_data_impl(compressAsFloat, tIns, tOuts, checksum, tempOf(tempMem, dev), outStatus, outSizes);
}

int64_t decompress_data_split_size(
    bool compressAsFloat, const std::vector<at::Tensor>& tIns, at::Tensor& tOut, const at::Tensor& tSplitSizes,
    bool checksum, const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& outStatus,
    const std::optional<at::Tensor>& outSizes) {
  TORCH_CHECK(!tIns.empty());
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  Temp tmp = tempOf(tempMem, dev);
  auto numInBatch = tSplitSizes.numel();
  TORCH_CHECK(tSplitSizes.is_contiguous());
  TORCH_CHECK(tSplitSizes.device().is_cpu());
  TORCH_CHECK(tSplitSizes.dtype() == at::kInt);
  TORCH_CHECK(numInBatch == (int64_t)tIns.size());
  std::vector<const void*> inPtrs(numInBatch);
  std::vector<uint32_t> splitSizes(numInBatch);
  std::vector<uint32_t> inBytes(numInBatch);
  for (int64_t i = 0; i < numInBatch; ++i) {
    auto& tIn = tIns[i];
    TORCH_CHECK(tIn.device().is_cuda());
    TORCH_CHECK(tIn.get_device() == dev);
    TORCH_CHECK(tIn.is_contiguous());
    TORCH_CHECK(tIn.dtype() == at::kByte);
    inPtrs[i] = tIn.data_ptr();
    inBytes[i] = (uint32_t)std::min<int64_t>(tIn.numel(), std::numeric_limits<uint32_t>::max());
    auto size = ((const int32_t*)tSplitSizes.data_ptr())[i];
    TORCH_CHECK(size > 0);
    splitSizes[i] = size;
  }
  TORCH_CHECK(tOut.device().is_cuda());
  TORCH_CHECK(tOut.get_device() == dev);
  TORCH_CHECK(tOut.is_contiguous());
  if (compressAsFloat) floatTypeFromDtype(tOut.scalar_type());
  validateStatus(outStatus, outSizes, numInBatch, dev);
  size_t used = 0;
  int32_t err = -1;
  if (compressAsFloat) {
    check(dgpu_float_decompress_split_size_bounded(tmp.ptr, tmp.bytes, &used, floatTypeFromDtype(tOut.scalar_type()),
                                           precision(), checksum, (uint32_t)numInBatch, inPtrs.data(), inBytes.data(),
                                           tOut.data_ptr(), splitSizes.data(),
                                           ptrOrNull<uint8_t>(outStatus), ptrOrNull<uint32_t>(outSizes), streamOf(dev), &err),
          "floatDecompressSplitSize", true);
  } else {
    check(dgpu_ans_decode_batch_split_size_bounded(tmp.ptr, tmp.bytes, &used, precision(), checksum, (uint32_t)numInBatch,
                                           inPtrs.data(), inBytes.data(), tOut.data_ptr(), splitSizes.data(),
                                           ptrOrNull<uint8_t>(outStatus), ptrOrNull<uint32_t>(outSizes), streamOf(dev), &err),
          "ansDecodeBatchSplitSize", false);
  }
  return (int64_t)used;
}

std::vector<at::Tensor> decompress_data_simple(
    bool compressAsFloat, const std::vector<at::Tensor>& tIns, bool checksum, const std::optional<int64_t>& tempMem) {
  TORCH_CHECK(!tIns.empty());
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  const size_t n = tIns.size();
  at::Tensor scratch;
  Temp tmp;
  if (tempMem && *tempMem >= 256) {  // kSDMAlignment, DietGpu.cpp:831-834
    scratch = at::empty({*tempMem}, at::TensorOptions().device(tIns[0].device()).dtype(at::kByte));
    tmp.ptr = scratch.data_ptr();
    tmp.bytes = (size_t)*tempMem;
  }
  std::vector<const void*> inPtrs(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(tIns[i].device().is_cuda());
    TORCH_CHECK(tIns[i].get_device() == dev);
    TORCH_CHECK(tIns[i].is_contiguous());
    inPtrs[i] = tIns[i].data_ptr();
  }
  auto opts = at::TensorOptions().device(tIns[0].device()).dtype(at::kInt);
  at::Tensor sizes = at::empty({(int64_t)n}, opts), types = at::zeros({(int64_t)n}, opts);
  if (compressAsFloat) {
    check(dgpu_float_get_compressed_info(tmp.ptr, tmp.bytes, inPtrs.data(), (uint32_t)n, (uint32_t*)sizes.data_ptr(),
                                         (uint32_t*)types.data_ptr(), nullptr, streamOf(dev)),
          "floatGetCompressedInfo", true);
  } else {
    check(dgpu_ans_get_compressed_info(tmp.ptr, tmp.bytes, inPtrs.data(), (uint32_t)n, (uint32_t*)sizes.data_ptr(),
                                       nullptr, streamOf(dev)),
          "ansGetCompressedInfo", false);
  }
  at::Tensor hs = sizes.to(at::kCPU), ht = types.to(at::kCPU);
  std::vector<at::Tensor> tOuts;
  for (size_t i = 0; i < n; ++i) {
    auto size = ((const int32_t*)hs.data_ptr())[i];
    auto type = ((const int32_t*)ht.data_ptr())[i];
    if (compressAsFloat) {
      TORCH_CHECK(type == ((const int32_t*)ht.data_ptr())[0]);  // must be a consistent dtype
      tOuts.emplace_back(at::empty({size}, at::TensorOptions().device(tIns[0].device()).dtype(dtypeFromFloatType(type))));
    } else {
      tOuts.emplace_back(at::empty({size}, at::TensorOptions().device(tIns[0].device()).dtype(at::kByte)));
    }
  }
  decompress_data_impl(compressAsFloat, tIns, tOuts, checksum, tmp, std::nullopt, std::nullopt);
  return tOuts;
}

// Ranged decode (no reference op): blocks [first_block[i], first_block[i] + num_blocks[i]) of archive i into ts_out[i],
// which holds the range (dgpu_ans_decode_batch_pointer_range / dgpu_float_decompress_range).  num_blocks[i] < 0 or
// >= 2^32 - 1 means "to the end of the element".  No checksum argument: a checksum covers the whole element.
int64_t decompress_data_range(
    bool compressAsFloat, const std::vector<at::Tensor>& tIns, const std::vector<at::Tensor>& tOuts,
    const std::vector<int64_t>& firstBlock, const std::vector<int64_t>& numBlocks, const std::optional<at::Tensor>& tempMem,
    const std::optional<at::Tensor>& outStatus, const std::optional<at::Tensor>& outSizes) {
  TORCH_CHECK(!tIns.empty());
  TORCH_CHECK(tIns.size() == tOuts.size());
  TORCH_CHECK(tIns.size() == firstBlock.size() && tIns.size() == numBlocks.size(), "dietgpu: one first_block and num_blocks per tensor");
  TORCH_CHECK(tIns.front().device().is_cuda());
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  Temp tmp = tempOf(tempMem, dev);
  const size_t n = tIns.size();
  std::vector<uint32_t> first(n), count(n);
  DecodeTensors m = marshalDecode(compressAsFloat, tIns, tOuts, dev, [&](size_t i) {
    if (compressAsFloat) TORCH_CHECK(tOuts[i].scalar_type() == tOuts[0].scalar_type());
    TORCH_CHECK(firstBlock[i] >= 0 && firstBlock[i] <= (int64_t)std::numeric_limits<uint32_t>::max(), "dietgpu: first_block out of range");
    first[i] = (uint32_t)firstBlock[i];
    const bool toEnd = numBlocks[i] < 0 || numBlocks[i] >= (int64_t)std::numeric_limits<uint32_t>::max();
    count[i] = toEnd ? std::numeric_limits<uint32_t>::max() : (uint32_t)numBlocks[i];
  });
  validateStatus(outStatus, outSizes, (int64_t)n, dev);
  size_t used = 0;
  uint8_t* status = ptrOrNull<uint8_t>(outStatus);
  uint32_t* sizes = ptrOrNull<uint32_t>(outSizes);
  if (compressAsFloat) {
    check(dgpu_float_decompress_range(tmp.ptr, tmp.bytes, &used, floatTypeFromDtype(tOuts[0].scalar_type()), precision(), (uint32_t)n,
                                      m.inPtrs.data(), m.inBytes.data(), first.data(), count.data(), m.outPtrs.data(),
                                      m.outCapacity.data(), status, sizes, streamOf(dev)),
          "floatDecompressRange", true);
  } else {
    check(dgpu_ans_decode_batch_pointer_range(tmp.ptr, tmp.bytes, &used, precision(), (uint32_t)n, m.inPtrs.data(), m.inBytes.data(),
                                              first.data(), count.data(), m.outPtrs.data(), m.outCapacity.data(), status, sizes,
                                              streamOf(dev)),
          "ansDecodeBatchPointerRange", false);
  }
  return (int64_t)used;
}

// Decode-accumulate (no reference op): archive i widened to float32 and stored to (accumulate = false) or added into
// ts_acc[i], a float32 tensor (dgpu_float_decode_accumulate).  float_type: what the archives hold (1 / 2 / 3).
int64_t decompress_data_accumulate(
    const std::vector<at::Tensor>& tIns, const std::vector<at::Tensor>& tAccs, int64_t floatType, bool accumulate,
    const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& outStatus, const std::optional<at::Tensor>& outSizes) {
  TORCH_CHECK(!tIns.empty());
  TORCH_CHECK(tIns.size() == tAccs.size());
  TORCH_CHECK(tIns.front().device().is_cuda(), "dietgpu: tensors must be on the GPU");
  TORCH_CHECK(floatType >= (int64_t)DGPU_FLOAT16 && floatType <= (int64_t)DGPU_FLOAT32, "dietgpu: float_type must be 1, 2 or 3");
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  Temp tmp = tempOf(tempMem, dev);
  const size_t n = tIns.size();
  DecodeTensors m = marshalDecode(true, tIns, tAccs, dev, [&](size_t i) {
    TORCH_CHECK(tAccs[i].scalar_type() == at::ScalarType::Float, "dietgpu: accumulators must be float32");
  });
  validateStatus(outStatus, outSizes, (int64_t)n, dev);
  size_t used = 0;
  check(dgpu_float_decode_accumulate(tmp.ptr, tmp.bytes, &used, (uint32_t)floatType, precision(), accumulate ? 1 : 0, (uint32_t)n,
                                         m.inPtrs.data(), m.inBytes.data(), m.outPtrs.data(), m.outCapacity.data(),
                                         ptrOrNull<uint8_t>(outStatus), ptrOrNull<uint32_t>(outSizes), streamOf(dev)),
        "floatDecompressAccumulate", true);
  return (int64_t)used;
}

// A tensor factor of the scaled decode calls: a float32 tensor on the tensors' GPU with 1 element (stride 0) or one per
// archive (stride 1).  The kernel reads it; nothing here does.  No tensor: null, the call's host float is used.
static const float* scaleFactors(const std::optional<at::Tensor>& scaleDev, size_t n, int dev, uint32_t* stride) {
  *stride = 0;
  if (!scaleDev) return nullptr;
  const at::Tensor& s = *scaleDev;
  TORCH_CHECK(s.device().is_cuda() && s.get_device() == dev && s.is_contiguous() && s.scalar_type() == at::ScalarType::Float,
              "dietgpu: a tensor scale must be a contiguous float32 tensor on the tensors' GPU");
  TORCH_CHECK(s.numel() == 1 || s.numel() == (int64_t)n, "dietgpu: a tensor scale holds 1 element or one per archive");
  *stride = (s.numel() == 1) ? 0u : 1u;
  return (const float*)s.data_ptr();
}

// Scaled decode-accumulate (no reference op): decompress_data_accumulate whose every widened word is multiplied by a
// float32 factor before it is stored or added (dgpu_float_decode_accumulate_scaled).  scale_dev as in
// decompress_data_scaled; without it: `scale`.
int64_t decompress_data_accumulate_scaled(
    const std::vector<at::Tensor>& tIns, const std::vector<at::Tensor>& tAccs, int64_t floatType, bool accumulate, double scale,
    const std::optional<at::Tensor>& scaleDev, const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& outStatus,
    const std::optional<at::Tensor>& outSizes) {
  TORCH_CHECK(!tIns.empty());
  TORCH_CHECK(tIns.size() == tAccs.size());
  TORCH_CHECK(tIns.front().device().is_cuda(), "dietgpu: tensors must be on the GPU");
  TORCH_CHECK(floatType >= (int64_t)DGPU_FLOAT16 && floatType <= (int64_t)DGPU_FLOAT32, "dietgpu: float_type must be 1, 2 or 3");
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  Temp tmp = tempOf(tempMem, dev);
  const size_t n = tIns.size();
  DecodeTensors m = marshalDecode(true, tIns, tAccs, dev, [&](size_t i) {
    TORCH_CHECK(tAccs[i].scalar_type() == at::ScalarType::Float, "dietgpu: accumulators must be float32");
  });
  uint32_t stride = 0;
  const float* factors = scaleFactors(scaleDev, n, dev, &stride);
  validateStatus(outStatus, outSizes, (int64_t)n, dev);
  size_t used = 0;
  check(dgpu_float_decode_accumulate_scaled(tmp.ptr, tmp.bytes, &used, (uint32_t)floatType, precision(), accumulate ? 1 : 0, (uint32_t)n,
                                                m.inPtrs.data(), m.inBytes.data(), m.outPtrs.data(), m.outCapacity.data(), (float)scale,
                                                factors, stride, ptrOrNull<uint8_t>(outStatus), ptrOrNull<uint32_t>(outSizes), streamOf(dev)),
        "floatDecompressAccumulateScaled", true);
  return (int64_t)used;
}

// Scaled decompress (no reference op): the float decode of archive i into ts_out[i] with every word multiplied by a
// float32 factor before it is stored (dgpu_float_decode_scaled).  scale_dev: a float32 tensor on the tensors' GPU
// with 1 element (one factor) or one per archive; the kernel reads it, nothing here does.  Without it: `scale`.
int64_t decompress_data_scaled(
    const std::vector<at::Tensor>& tIns, const std::vector<at::Tensor>& tOuts, double scale, const std::optional<at::Tensor>& scaleDev,
    const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& outStatus, const std::optional<at::Tensor>& outSizes) {
  TORCH_CHECK(!tIns.empty());
  TORCH_CHECK(tIns.size() == tOuts.size());
  TORCH_CHECK(tIns.front().device().is_cuda(), "dietgpu: tensors must be on the GPU");
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  Temp tmp = tempOf(tempMem, dev);
  const size_t n = tIns.size();
  DecodeTensors m = marshalDecode(true, tIns, tOuts, dev, [&](size_t i) {
    TORCH_CHECK(tOuts[i].scalar_type() == tOuts[0].scalar_type(), "dietgpu: outputs must share one float dtype");
  });
  uint32_t stride = 0;
  const float* factors = scaleFactors(scaleDev, n, dev, &stride);
  validateStatus(outStatus, outSizes, (int64_t)n, dev);
  size_t used = 0;
  check(dgpu_float_decode_scaled(tmp.ptr, tmp.bytes, &used, floatTypeFromDtype(tOuts[0].scalar_type()), precision(), (uint32_t)n,
                                     m.inPtrs.data(), m.inBytes.data(), m.outPtrs.data(), m.outCapacity.data(), (float)scale, factors,
                                     stride, ptrOrNull<uint8_t>(outStatus), ptrOrNull<uint32_t>(outSizes), streamOf(dev)),
        "floatDecompressScaled", true);
  return (int64_t)used;
}

// Decode-update (no reference op): archive i multiplied by a float32 factor, added to (accumulate) or stored over the
// 16-bit tensor ts_out[i] of the archive's type and rounded stochastically (dgpu_float_decode_update).  scale_dev as in
// decompress_data_scaled.  seed: the 64 seed bits as an int64; seed_dev: a 1-element int64 tensor on the tensors' GPU
// whose bits are the seed -- the kernel reads it, nothing here does.  -> 0 (the call uses no temp memory).
int64_t decompress_data_update(
    const std::vector<at::Tensor>& tIns, const std::vector<at::Tensor>& tOuts, double scale, const std::optional<at::Tensor>& scaleDev,
    int64_t seed, const std::optional<at::Tensor>& seedDev, int64_t firstMember, bool accumulate,
    const std::optional<at::Tensor>& outStatus, const std::optional<at::Tensor>& outSizes) {
  TORCH_CHECK(!tIns.empty());
  TORCH_CHECK(tIns.size() == tOuts.size());
  TORCH_CHECK(tIns.front().device().is_cuda(), "dietgpu: tensors must be on the GPU");
  TORCH_CHECK(firstMember >= 0 && firstMember <= (int64_t)std::numeric_limits<uint32_t>::max(), "dietgpu: first_member must be in [0, 2^32)");
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  const size_t n = tIns.size();
  DecodeTensors m = marshalDecode(true, tIns, tOuts, dev, [&](size_t i) {
    TORCH_CHECK(tOuts[i].scalar_type() == tOuts[0].scalar_type(), "dietgpu: outputs must share one float dtype");
  });
  TORCH_CHECK(tOuts[0].scalar_type() == at::ScalarType::Half || tOuts[0].scalar_type() == at::ScalarType::BFloat16,
              "dietgpu: decode-update takes float16 or bfloat16 tensors");
  uint32_t stride = 0;
  const float* factors = scaleFactors(scaleDev, n, dev, &stride);
  const uint64_t* seedPtr = nullptr;
  if (seedDev) {
    const at::Tensor& s = *seedDev;
    TORCH_CHECK(s.device().is_cuda() && s.get_device() == dev && s.is_contiguous() && s.scalar_type() == at::ScalarType::Long && s.numel() == 1,
                "dietgpu: a tensor seed must be a 1-element int64 tensor on the tensors' GPU");
    seedPtr = (const uint64_t*)s.data_ptr();
  }
  validateStatus(outStatus, outSizes, (int64_t)n, dev);
  check(dgpu_float_decode_update(floatTypeFromDtype(tOuts[0].scalar_type()), precision(), accumulate ? 1 : 0, (uint32_t)n, m.inPtrs.data(),
                                 m.inBytes.data(), m.outPtrs.data(), m.outCapacity.data(), (float)scale, factors, stride, (uint64_t)seed,
                                 seedPtr, (uint32_t)firstMember, ptrOrNull<uint8_t>(outStatus), ptrOrNull<uint32_t>(outSizes), streamOf(dev)),
        "floatDecompressUpdate", true);
  return 0;
}

// Cast-compress (no reference op): float32 tensor i rounded to float_type (1 = float16, 2 = bfloat16) in registers and
// compressed into an ordinary archive of that type (dgpu_float_cast_compress).  Output conventions of compress_data.
std::tuple<at::Tensor, at::Tensor, int64_t> compress_data_cast(
    const std::vector<at::Tensor>& tIns, int64_t floatType, const std::optional<at::Tensor>& tempMem,
    const std::optional<at::Tensor>& outCompressed, const std::optional<at::Tensor>& outCompressedSizes) {
  TORCH_CHECK(!tIns.empty());
  TORCH_CHECK(tIns.front().device().is_cuda(), "dietgpu: tensors must be on the GPU");
  TORCH_CHECK(floatType == (int64_t)DGPU_FLOAT16 || floatType == (int64_t)DGPU_BFLOAT16, "dietgpu: float_type must be 1 (float16) or 2 (bfloat16)");
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  Temp tmp = tempOf(tempMem, dev);
  const size_t n = tIns.size();
  int64_t maxWords = 0;
  for (auto& t : tIns) {
    TORCH_CHECK(t.device().is_cuda());
    TORCH_CHECK(t.is_contiguous());
    TORCH_CHECK(t.get_device() == dev);
    TORCH_CHECK(t.scalar_type() == at::ScalarType::Float, "dietgpu: the inputs of a cast call must be float32");
    maxWords = std::max<int64_t>(maxWords, t.numel());
  }
  at::Tensor comp, sizes;
  validateCompOut(outCompressed, outCompressedSizes, (int64_t)n, (int64_t)maxFloatSize((uint32_t)floatType, (uint64_t)maxWords), dev,
                  tIns[0].device(), comp, sizes);
  std::vector<const void*> inPtrs(n);
  std::vector<uint32_t> inSize(n);
  std::vector<void*> compPtrs(n);
  for (size_t i = 0; i < n; ++i) {
    inPtrs[i] = tIns[i].data_ptr();
    inSize[i] = (uint32_t)tIns[i].numel();
    compPtrs[i] = (uint8_t*)comp.data_ptr() + i * comp.size(1);
  }
  size_t used = 0;
  check(dgpu_float_cast_compress(tmp.ptr, tmp.bytes, &used, (uint32_t)floatType, precision(), (uint32_t)n, inPtrs.data(), inSize.data(),
                                 compPtrs.data(), (uint32_t*)sizes.data_ptr(), streamOf(dev)),
        "floatCompressCast", true);
  return {std::move(comp), std::move(sizes), (int64_t)used};
}

// Feedback cast-compress (no reference op): compress_data_cast of ts_in[i] + ts_residual[i], with ts_residual[i] --
// float32, of the tensor's size -- updated in place to the rounding error (dgpu_float_feedback_compress).  fresh: no
// residual yet, the buffers are only written.
std::tuple<at::Tensor, at::Tensor, int64_t> compress_data_feedback(
    const std::vector<at::Tensor>& tIns, const std::vector<at::Tensor>& tResiduals, int64_t floatType, bool fresh,
    const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& outCompressed, const std::optional<at::Tensor>& outCompressedSizes) {
  TORCH_CHECK(!tIns.empty());
  TORCH_CHECK(tIns.size() == tResiduals.size(), "dietgpu: one residual per tensor");
  TORCH_CHECK(tIns.front().device().is_cuda(), "dietgpu: tensors must be on the GPU");
  TORCH_CHECK(floatType == (int64_t)DGPU_FLOAT16 || floatType == (int64_t)DGPU_BFLOAT16, "dietgpu: float_type must be 1 (float16) or 2 (bfloat16)");
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  Temp tmp = tempOf(tempMem, dev);
  const size_t n = tIns.size();
  int64_t maxWords = 0;
  for (size_t i = 0; i < n; ++i) {
    const at::Tensor &t = tIns[i], &r = tResiduals[i];
    TORCH_CHECK(t.device().is_cuda() && t.is_contiguous() && t.get_device() == dev);
    TORCH_CHECK(t.scalar_type() == at::ScalarType::Float, "dietgpu: the inputs of a feedback call must be float32");
    TORCH_CHECK(r.device().is_cuda() && r.is_contiguous() && r.get_device() == dev && r.scalar_type() == at::ScalarType::Float &&
                    r.numel() == t.numel(),
                "dietgpu: a residual is a contiguous float32 tensor of its tensor's size on its GPU");
    maxWords = std::max<int64_t>(maxWords, t.numel());
  }
  at::Tensor comp, sizes;
  validateCompOut(outCompressed, outCompressedSizes, (int64_t)n, (int64_t)maxFloatSize((uint32_t)floatType, (uint64_t)maxWords), dev,
                  tIns[0].device(), comp, sizes);
  std::vector<const void*> inPtrs(n), resIn(n);
  std::vector<uint32_t> inSize(n);
  std::vector<void*> compPtrs(n), resOut(n);
  for (size_t i = 0; i < n; ++i) {
    inPtrs[i] = tIns[i].data_ptr();
    inSize[i] = (uint32_t)tIns[i].numel();
    resIn[i] = resOut[i] = tResiduals[i].data_ptr();
    compPtrs[i] = (uint8_t*)comp.data_ptr() + i * comp.size(1);
  }
  size_t used = 0;
  check(dgpu_float_feedback_compress(tmp.ptr, tmp.bytes, &used, (uint32_t)floatType, precision(), (uint32_t)n, inPtrs.data(), inSize.data(),
                                     fresh ? nullptr : resIn.data(), resOut.data(), compPtrs.data(), (uint32_t*)sizes.data_ptr(), streamOf(dev)),
        "floatCompressFeedback", true);
  return {std::move(comp), std::move(sizes), (int64_t)used};
}

// Stochastic cast-compress (no reference op): compress_data_cast whose every rounding is stochastic, with the random bits of
// (seed, first_member + i, word index) (dgpu_float_stochastic_compress).  seed / seed_dev as in decompress_data_update.  No
// temp memory is passed: -> (comp, sizes).
std::tuple<at::Tensor, at::Tensor> compress_data_stochastic(
    const std::vector<at::Tensor>& tIns, int64_t floatType, int64_t seed, const std::optional<at::Tensor>& seedDev, int64_t firstMember,
    const std::optional<at::Tensor>& outCompressed, const std::optional<at::Tensor>& outCompressedSizes) {
  TORCH_CHECK(!tIns.empty());
  TORCH_CHECK(tIns.front().device().is_cuda(), "dietgpu: tensors must be on the GPU");
  TORCH_CHECK(floatType == (int64_t)DGPU_FLOAT16 || floatType == (int64_t)DGPU_BFLOAT16, "dietgpu: float_type must be 1 (float16) or 2 (bfloat16)");
  TORCH_CHECK(firstMember >= 0 && firstMember <= (int64_t)std::numeric_limits<uint32_t>::max(), "dietgpu: first_member must be in [0, 2^32)");
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  const size_t n = tIns.size();
  int64_t maxWords = 0;
  for (auto& t : tIns) {
    TORCH_CHECK(t.device().is_cuda() && t.is_contiguous() && t.get_device() == dev);
    TORCH_CHECK(t.scalar_type() == at::ScalarType::Float, "dietgpu: the inputs of a stochastic cast call must be float32");
    maxWords = std::max<int64_t>(maxWords, t.numel());
  }
  const uint64_t* seedPtr = nullptr;
  if (seedDev) {
    const at::Tensor& s = *seedDev;
    TORCH_CHECK(s.device().is_cuda() && s.get_device() == dev && s.is_contiguous() && s.scalar_type() == at::ScalarType::Long && s.numel() == 1,
                "dietgpu: a tensor seed must be a 1-element int64 tensor on the tensors' GPU");
    seedPtr = (const uint64_t*)s.data_ptr();
  }
  at::Tensor comp, sizes;
  validateCompOut(outCompressed, outCompressedSizes, (int64_t)n, (int64_t)maxFloatSize((uint32_t)floatType, (uint64_t)maxWords), dev,
                  tIns[0].device(), comp, sizes);
  std::vector<const void*> inPtrs(n);
  std::vector<uint32_t> inSize(n);
  std::vector<void*> compPtrs(n);
  for (size_t i = 0; i < n; ++i) {
    inPtrs[i] = tIns[i].data_ptr();
    inSize[i] = (uint32_t)tIns[i].numel();
    compPtrs[i] = (uint8_t*)comp.data_ptr() + i * comp.size(1);
  }
  check(dgpu_float_stochastic_compress((uint32_t)floatType, precision(), (uint32_t)n, inPtrs.data(), inSize.data(), (uint64_t)seed, seedPtr,
                                       (uint32_t)firstMember, compPtrs.data(), (uint32_t*)sizes.data_ptr(), streamOf(dev)),
        "floatCompressStochastic", true);
  return {std::move(comp), std::move(sizes)};
}

// Rolling-table compress (no reference op): compress_data / compress_data_cast with the tables made from the counts the
// last call left (counts_in) and this call's counts taken by the encoder (counts_out): dgpu_float_rolling_compress.
// float_type (1 = float16, 2 = bfloat16) is that of the archives; source_float32: ts_in are float32 and are rounded.
std::tuple<at::Tensor, at::Tensor, int64_t> compress_data_rolling(
    const std::vector<at::Tensor>& tIns, const std::optional<at::Tensor>& countsIn, const std::optional<at::Tensor>& countsOut,
    int64_t floatType, bool sourceFloat32, const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& outCompressed,
    const std::optional<at::Tensor>& outCompressedSizes) {
  TORCH_CHECK(!tIns.empty());
  TORCH_CHECK(tIns.front().device().is_cuda(), "dietgpu: tensors must be on the GPU");
  TORCH_CHECK(floatType == (int64_t)DGPU_FLOAT16 || floatType == (int64_t)DGPU_BFLOAT16, "dietgpu: float_type must be 1 (float16) or 2 (bfloat16)");
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  Temp tmp = tempOf(tempMem, dev);
  const size_t n = tIns.size();
  const at::ScalarType want = sourceFloat32 ? at::ScalarType::Float : dtypeFromFloatType((uint32_t)floatType);
  int64_t maxWords = 0;
  for (auto& t : tIns) {
    TORCH_CHECK(t.device().is_cuda());
    TORCH_CHECK(t.is_contiguous());
    TORCH_CHECK(t.get_device() == dev);
    TORCH_CHECK(t.scalar_type() == want, "dietgpu: the inputs must be float32 (source_float32) or of the archives' type");
    maxWords = std::max<int64_t>(maxWords, t.numel());
  }
  for (const std::optional<at::Tensor>* c : {&countsIn, &countsOut}) {
    if (!*c) continue;
    TORCH_CHECK((*c)->device().is_cuda() && (*c)->get_device() == dev && (*c)->is_contiguous() && (*c)->scalar_type() == at::kInt,
                "dietgpu: counts must be contiguous int32 tensors on the tensors' GPU");
    TORCH_CHECK((*c)->dim() == 2 && (*c)->size(0) == (int64_t)n && (*c)->size(1) == 256, "dietgpu: counts must be [len(ts_in), 256]");
  }
  at::Tensor comp, sizes;
  validateCompOut(outCompressed, outCompressedSizes, (int64_t)n, (int64_t)maxFloatSize((uint32_t)floatType, (uint64_t)maxWords), dev,
                  tIns[0].device(), comp, sizes);
  std::vector<const void*> inPtrs(n);
  std::vector<uint32_t> inSize(n);
  std::vector<void*> compPtrs(n);
  for (size_t i = 0; i < n; ++i) {
    inPtrs[i] = tIns[i].data_ptr();
    inSize[i] = (uint32_t)tIns[i].numel();
    compPtrs[i] = (uint8_t*)comp.data_ptr() + i * comp.size(1);
  }
  size_t used = 0;
  check(dgpu_float_rolling_compress(tmp.ptr, tmp.bytes, &used, (uint32_t)floatType, sourceFloat32 ? 1u : 0u, precision(), (uint32_t)n,
                                    inPtrs.data(), inSize.data(), ptrOrNull<const uint32_t>(countsIn), ptrOrNull<uint32_t>(countsOut),
                                    compPtrs.data(), (uint32_t*)sizes.data_ptr(), streamOf(dev)),
        "floatCompressRolling", true);
  return {std::move(comp), std::move(sizes), (int64_t)used};
}

// The reduce family (no reference ops): num_sources sources per accumulator, ts_in flattened member-major (source s of
// accumulator i is ts_in[i * num_sources + s]), summed left to right in one launch, all or nothing per accumulator;
// accumulate = false stores the first source: the accumulators are never read.  Eight ops over one implementation:
//   * decompress_data_reduce{,_mixed,_scaled,_norm} leave the sums in ts_acc (float_type 1 / 2 / 3);
//   * decompress_data_reduce_compress{,_mixed,_scaled,_norm} also compress_data_cast them in the same call (float_type 1 =
//     float16 or 2 = bfloat16, of the sources and of the archives; output conventions of compress_data_cast);
//   * plain: every source is a uint8 archive.  The others: a uint8 tensor is an archive, a tensor of the dtype float_type
//     names a RAW row (1-D, contiguous, on the device), anything else an error;
//   * _scaled: the sums are multiplied by `scale` in the reduce kernel -- a float32 value (ops.py rounds it once), finite
//     and not zero, as the C ABI demands;
//   * _norm: the scaled ops that also report, per accumulator, the squared norm (float64) and the non-finite count (int32)
//     of what the call leaves.  A scale of 1.0 is no scale.  Either output may be absent; with both absent the call is
//     the scaled one.
namespace {
enum class Reduce { kPlain, kMixed, kScaled, kNorm };
const std::optional<at::Tensor> kAbsent;

struct ReduceTensors {
  std::vector<const void*> inPtrs;
  std::vector<uint32_t> inBytes;
  std::vector<uint8_t> kinds;
  std::vector<void*> accPtrs;
  std::vector<uint32_t> capacity;
  int64_t maxWords = 0;
};
ReduceTensors marshalReduce(const std::vector<at::Tensor>& tIns, const std::vector<at::Tensor>& tAccs, int64_t floatType, int dev, bool rawAllowed) {
  const at::ScalarType rawType = floatType == (int64_t)DGPU_FLOAT16 ? at::ScalarType::Half
      : (floatType == (int64_t)DGPU_BFLOAT16 ? at::ScalarType::BFloat16 : at::ScalarType::Float);
  const size_t n = tAccs.size();
  ReduceTensors m;
  m.inPtrs.resize(tIns.size());
  m.inBytes.resize(tIns.size());
  m.kinds.resize(tIns.size());
  m.accPtrs.resize(n);
  m.capacity.resize(n);
  for (size_t k = 0; k < tIns.size(); ++k) {
    auto& t = tIns[k];
    TORCH_CHECK(t.device().is_cuda() && t.get_device() == dev && t.is_contiguous(), "dietgpu: sources must be contiguous tensors on one GPU");
    const bool raw = t.scalar_type() != at::ScalarType::Byte;
    TORCH_CHECK(!raw || rawAllowed, "dietgpu: a source must be a uint8 archive");
    TORCH_CHECK(!raw || t.scalar_type() == rawType, "dietgpu: a source is a uint8 archive or a raw row of the dtype float_type names");
    TORCH_CHECK(!raw || t.dim() == 1, "dietgpu: a raw source must be 1-D");
    const int64_t bytes = t.numel() * (int64_t)t.element_size();
    TORCH_CHECK(!raw || bytes <= (int64_t)std::numeric_limits<uint32_t>::max(), "dietgpu: raw source too large");
    m.inPtrs[k] = t.data_ptr();
    m.inBytes[k] = (uint32_t)std::min<int64_t>(bytes, std::numeric_limits<uint32_t>::max());
    m.kinds[k] = raw ? 1 : 0;
  }
  for (size_t i = 0; i < n; ++i) {
    auto& t = tAccs[i];
    TORCH_CHECK(t.device().is_cuda() && t.get_device() == dev && t.is_contiguous(), "dietgpu: accumulators must be contiguous tensors on the GPU");
    TORCH_CHECK(t.scalar_type() == at::ScalarType::Float, "dietgpu: accumulators must be float32");
    TORCH_CHECK((uint64_t)t.numel() <= std::numeric_limits<uint32_t>::max());
    m.accPtrs[i] = t.data_ptr();
    m.capacity[i] = (uint32_t)t.numel();
    m.maxWords = std::max<int64_t>(m.maxWords, t.numel());
  }
  return m;
}

void validateNorm(const std::optional<at::Tensor>& outSumSq, const std::optional<at::Tensor>& outNonFinite, int64_t n, int dev) {
  if (outSumSq) {
    TORCH_CHECK(outSumSq->scalar_type() == at::ScalarType::Double, "dietgpu: out_sumsq must be a float64 tensor");
    TORCH_CHECK(outSumSq->dim() == 1 && outSumSq->numel() == n && outSumSq->is_contiguous(), "dietgpu: out_sumsq must be a contiguous tensor with one entry per accumulator");
    TORCH_CHECK(outSumSq->device().is_cuda() && outSumSq->get_device() == dev, "dietgpu: out_sumsq must be on the GPU of the other tensors");
  }
  if (outNonFinite) {
    TORCH_CHECK(outNonFinite->scalar_type() == at::ScalarType::Int, "dietgpu: out_nonfinite must be an int32 tensor");
    TORCH_CHECK(outNonFinite->dim() == 1 && outNonFinite->numel() == n && outNonFinite->is_contiguous(), "dietgpu: out_nonfinite must be a contiguous tensor with one entry per accumulator");
    TORCH_CHECK(outNonFinite->device().is_cuda() && outNonFinite->get_device() == dev, "dietgpu: out_nonfinite must be on the GPU of the other tensors");
  }
}

// -> (comp, sizes, temp bytes used); without `compress` the two tensors are undefined.
std::tuple<at::Tensor, at::Tensor, int64_t> reduceCall(
    Reduce kind, bool compress, const std::vector<at::Tensor>& tIns, int64_t numSources, const std::vector<at::Tensor>& tAccs, int64_t floatType,
    double scale, bool accumulate, const std::optional<at::Tensor>& tempMem, const std::optional<at::Tensor>& outStatus,
    const std::optional<at::Tensor>& outSizes, const std::optional<at::Tensor>& outCompressed = kAbsent,
    const std::optional<at::Tensor>& outCompressedSizes = kAbsent, const std::optional<at::Tensor>& outSumSq = kAbsent,
    const std::optional<at::Tensor>& outNonFinite = kAbsent) {
  const float f = (float)scale;
  TORCH_CHECK(kind < Reduce::kScaled || (std::isfinite(f) && f != 0.0f), "dietgpu: scale must be finite and not zero");
  TORCH_CHECK(!tIns.empty() && !tAccs.empty());
  TORCH_CHECK(numSources >= 1 && numSources <= 64, "dietgpu: num_sources must be between 1 and 64");
  TORCH_CHECK(tIns.size() == tAccs.size() * (size_t)numSources, "dietgpu: ts_in holds num_sources tensors per accumulator");
  TORCH_CHECK(tIns.front().device().is_cuda(), "dietgpu: tensors must be on the GPU");
  if (compress) {
    TORCH_CHECK(floatType == (int64_t)DGPU_FLOAT16 || floatType == (int64_t)DGPU_BFLOAT16, "dietgpu: float_type must be 1 (float16) or 2 (bfloat16)");
  } else {
    TORCH_CHECK(floatType >= (int64_t)DGPU_FLOAT16 && floatType <= (int64_t)DGPU_FLOAT32, "dietgpu: float_type must be 1, 2 or 3");
  }
  int dev = tIns.front().get_device();
  c10::hip::HIPGuard guard(dev);
  Temp tmp = tempOf(tempMem, dev);
  const size_t n = tAccs.size();
  ReduceTensors m = marshalReduce(tIns, tAccs, floatType, dev, kind != Reduce::kPlain);
  validateStatus(outStatus, outSizes, (int64_t)n, dev);
  if (kind == Reduce::kNorm) validateNorm(outSumSq, outNonFinite, (int64_t)n, dev);
  at::Tensor comp, sizes;
  std::vector<void*> compPtrs(compress ? n : 0);
  if (compress) {
    validateCompOut(outCompressed, outCompressedSizes, (int64_t)n, (int64_t)maxFloatSize((uint32_t)floatType, (uint64_t)m.maxWords), dev,
                    tAccs[0].device(), comp, sizes);
    for (size_t i = 0; i < n; ++i) compPtrs[i] = (uint8_t*)comp.data_ptr() + i * comp.size(1);
  }
  size_t used = 0;
  const uint32_t ft = (uint32_t)floatType, B = (uint32_t)n, S = (uint32_t)numSources;
  const int P = precision(), acc = accumulate ? 1 : 0;
  const void* const* in = m.inPtrs.data();
  const uint32_t* inBytes = m.inBytes.data();
  const uint8_t* kinds = m.kinds.data();
  void* const* accs = m.accPtrs.data();
  const uint32_t* cap = m.capacity.data();
  uint8_t* status = ptrOrNull<uint8_t>(outStatus);
  uint32_t* words = ptrOrNull<uint32_t>(outSizes);
  uint32_t* archBytes = compress ? (uint32_t*)sizes.data_ptr() : nullptr;
  double* sumSq = ptrOrNull<double>(outSumSq);
  uint32_t* nonFinite = ptrOrNull<uint32_t>(outNonFinite);
  void* stream = streamOf(dev);
  // (each op calls the entry point of its own name)
  if (!compress) {
    switch (kind) {
      case Reduce::kPlain:
        check(dgpu_float_decode_reduce(tmp.ptr, tmp.bytes, &used, ft, P, acc, B, S, in, inBytes, accs, cap, status, words, stream), "floatDecompressReduce", true);
        break;
      case Reduce::kMixed:
        check(dgpu_float_decode_reduce_mixed(tmp.ptr, tmp.bytes, &used, ft, P, acc, B, S, in, inBytes, kinds, accs, cap, status, words, stream),
              "floatDecompressReduceMixed", true);
        break;
      case Reduce::kScaled:
        check(dgpu_float_decode_reduce_scaled(tmp.ptr, tmp.bytes, &used, ft, P, acc, B, S, in, inBytes, kinds, f, accs, cap, status, words, stream),
              "floatDecompressReduceScaled", true);
        break;
      case Reduce::kNorm:
        check(dgpu_float_decode_reduce_norm(tmp.ptr, tmp.bytes, &used, ft, P, acc, B, S, in, inBytes, kinds, f, accs, cap, status, words, sumSq, nonFinite, stream),
              "floatDecompressReduceNorm", true);
        break;
    }
  } else {
    void* const* arch = compPtrs.data();
    switch (kind) {
      case Reduce::kPlain:
        check(dgpu_float_reduce_compress(tmp.ptr, tmp.bytes, &used, ft, P, acc, B, S, in, inBytes, accs, cap, arch, status, words, archBytes, stream),
              "floatReduceCompress", true);
        break;
      case Reduce::kMixed:
        check(dgpu_float_reduce_compress_mixed(tmp.ptr, tmp.bytes, &used, ft, P, acc, B, S, in, inBytes, kinds, accs, cap, arch, status, words, archBytes, stream),
              "floatReduceCompressMixed", true);
        break;
      case Reduce::kScaled:
        check(dgpu_float_reduce_compress_scaled(tmp.ptr, tmp.bytes, &used, ft, P, acc, B, S, in, inBytes, kinds, f, accs, cap, arch, status, words, archBytes, stream),
              "floatReduceCompressScaled", true);
        break;
      case Reduce::kNorm:
        check(dgpu_float_reduce_compress_norm(tmp.ptr, tmp.bytes, &used, ft, P, acc, B, S, in, inBytes, kinds, f, accs, cap, arch, status, words, archBytes, sumSq,
                                              nonFinite, stream),
              "floatReduceCompressNorm", true);
        break;
    }
  }
  return {std::move(comp), std::move(sizes), (int64_t)used};
}
}  // namespace

using Tensors = std::vector<at::Tensor>;
using Opt = std::optional<at::Tensor>;
using Compressed = std::tuple<at::Tensor, at::Tensor, int64_t>;

int64_t decompress_data_reduce(const Tensors& tIns, int64_t numSources, const Tensors& tAccs, int64_t floatType, bool accumulate, const Opt& tempMem,
                               const Opt& outStatus, const Opt& outSizes) {
  return std::get<2>(reduceCall(Reduce::kPlain, false, tIns, numSources, tAccs, floatType, 1.0, accumulate, tempMem, outStatus, outSizes));
}
int64_t decompress_data_reduce_mixed(const Tensors& tIns, int64_t numSources, const Tensors& tAccs, int64_t floatType, bool accumulate, const Opt& tempMem,
                                     const Opt& outStatus, const Opt& outSizes) {
  return std::get<2>(reduceCall(Reduce::kMixed, false, tIns, numSources, tAccs, floatType, 1.0, accumulate, tempMem, outStatus, outSizes));
}
int64_t decompress_data_reduce_scaled(const Tensors& tIns, int64_t numSources, const Tensors& tAccs, int64_t floatType, double scale, bool accumulate,
                                      const Opt& tempMem, const Opt& outStatus, const Opt& outSizes) {
  return std::get<2>(reduceCall(Reduce::kScaled, false, tIns, numSources, tAccs, floatType, scale, accumulate, tempMem, outStatus, outSizes));
}
int64_t decompress_data_reduce_norm(const Tensors& tIns, int64_t numSources, const Tensors& tAccs, int64_t floatType, double scale, bool accumulate,
                                    const Opt& tempMem, const Opt& outStatus, const Opt& outSizes, const Opt& outSumSq, const Opt& outNonFinite) {
  return std::get<2>(reduceCall(Reduce::kNorm, false, tIns, numSources, tAccs, floatType, scale, accumulate, tempMem, outStatus, outSizes, kAbsent, kAbsent,
                                outSumSq, outNonFinite));
}
Compressed decompress_data_reduce_compress(const Tensors& tIns, int64_t numSources, const Tensors& tAccs, int64_t floatType, bool accumulate,
                                           const Opt& tempMem, const Opt& outStatus, const Opt& outSizes, const Opt& outCompressed,
                                           const Opt& outCompressedSizes) {
  return reduceCall(Reduce::kPlain, true, tIns, numSources, tAccs, floatType, 1.0, accumulate, tempMem, outStatus, outSizes, outCompressed, outCompressedSizes);
}
Compressed decompress_data_reduce_compress_mixed(const Tensors& tIns, int64_t numSources, const Tensors& tAccs, int64_t floatType, bool accumulate,
                                                 const Opt& tempMem, const Opt& outStatus, const Opt& outSizes, const Opt& outCompressed,
                                                 const Opt& outCompressedSizes) {
  return reduceCall(Reduce::kMixed, true, tIns, numSources, tAccs, floatType, 1.0, accumulate, tempMem, outStatus, outSizes, outCompressed, outCompressedSizes);
}
Compressed decompress_data_reduce_compress_scaled(const Tensors& tIns, int64_t numSources, const Tensors& tAccs, int64_t floatType, double scale,
                                                  bool accumulate, const Opt& tempMem, const Opt& outStatus, const Opt& outSizes,
                                                  const Opt& outCompressed, const Opt& outCompressedSizes) {
  return reduceCall(Reduce::kScaled, true, tIns, numSources, tAccs, floatType, scale, accumulate, tempMem, outStatus, outSizes, outCompressed, outCompressedSizes);
}
Compressed decompress_data_reduce_compress_norm(const Tensors& tIns, int64_t numSources, const Tensors& tAccs, int64_t floatType, double scale,
                                                bool accumulate, const Opt& tempMem, const Opt& outStatus, const Opt& outSizes, const Opt& outCompressed,
                                                const Opt& outCompressedSizes, const Opt& outSumSq, const Opt& outNonFinite) {
  return reduceCall(Reduce::kNorm, true, tIns, numSources, tAccs, floatType, scale, accumulate, tempMem, outStatus, outSizes, outCompressed, outCompressedSizes,
                    outSumSq, outNonFinite);
}

void set_precision(int64_t probBits) {
  TORCH_CHECK(probBits == 9 || probBits == 10 || probBits == 11, "probBits must be 9, 10 or 11");
  tPrecision = (int)probBits;
}

}  // namespace dietgpu_amd

// Schema strings verbatim from DietGpu.cpp:915-937
TORCH_LIBRARY_FRAGMENT(dietgpu, m) {
  m.def("max_float_compressed_output_size(Tensor[] ts) -> (int, int)");
  m.def("max_float_compressed_size(Tensor dtype, int size) -> int");
  m.def("max_any_compressed_output_size(Tensor[] ts) -> (int, int)");
  m.def("max_any_compressed_size(int bytes) -> int");
  m.def(
      "compress_data(bool compress_as_float, Tensor[] ts_in, bool checksum=False, Tensor? temp_mem=None, Tensor? out_compressed=None, Tensor? out_compressed_bytes=None) -> (Tensor, Tensor, int)");
  m.def(
      "compress_data_split_size(bool compress_as_float, Tensor t_in, Tensor t_in_split_sizes, bool checksum=False, Tensor? temp_mem=None, Tensor? out_compressed=None, Tensor? out_compressed_bytes=None) -> (Tensor[], Tensor, int)");
  m.def(
      "compress_data_simple(bool compress_as_float, Tensor[] ts_in, bool checksum=False, int? temp_mem=67108864) -> Tensor[]");
  m.def(
      "decompress_data(bool compress_as_float, Tensor[] ts_in, Tensor[] ts_out, bool checksum=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_decompressed_words=None) -> (int)");
  m.def(
      "decompress_data_split_size(bool compress_as_float, Tensor[] ts_in, Tensor t_out, Tensor t_out_split_sizes, bool checksum=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_decompressed_words=None) -> (int)");
  m.def(
      "decompress_data_simple(bool compress_as_float, Tensor[] ts_in, bool checksum=False, int? temp_mem=67108864) -> Tensor[]");
}

// The version of the C ABI this file was compiled against, and whether the ops below were registered.  Plain C symbols:
// dietgpu_amd/ops.py compares them through ctypes after loading the library.  Nothing here throws -- torch.ops.load_library
// is a dlopen, and a C++ exception leaving a static initialiser under dlopen ends in std::terminate, not in Python.
extern "C" uint32_t dgpu_torch_built_abi(void) { return DGPU_ABI_VERSION; }
static bool gOpsRegistered = false;
extern "C" int dgpu_torch_ops_registered(void) { return gOpsRegistered ? 1 : 0; }
// a libdietgpu_amd.so from another build of the sources than this file was compiled against: register nothing
static bool coreLibraryMatches() { return dgpu_abi_version() == DGPU_ABI_VERSION; }

TORCH_LIBRARY(dietgpu_amd, m) {
  if (!coreLibraryMatches()) return;
  m.def("set_precision(int prob_bits) -> ()", &dietgpu_amd::set_precision);
  m.def(
      "decompress_data_range(bool compress_as_float, Tensor[] ts_in, Tensor[] ts_out, int[] first_block, int[] num_blocks, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_decompressed_words=None) -> int",
      &dietgpu_amd::decompress_data_range);
  m.def(
      "decompress_data_accumulate(Tensor[] ts_in, Tensor[] ts_acc, int float_type, bool accumulate=True, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_sizes=None) -> int",
      &dietgpu_amd::decompress_data_accumulate);
  m.def(
      "decompress_data_accumulate_scaled(Tensor[] ts_in, Tensor[] ts_acc, int float_type, bool accumulate, float scale, Tensor? scale_dev=None, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_sizes=None) -> int",
      &dietgpu_amd::decompress_data_accumulate_scaled);
  m.def(
      "decompress_data_scaled(Tensor[] ts_in, Tensor[] ts_out, float scale, Tensor? scale_dev=None, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_decompressed_words=None) -> int",
      &dietgpu_amd::decompress_data_scaled);
  m.def(
      "decompress_data_update(Tensor[] ts_in, Tensor[] ts_out, float scale, Tensor? scale_dev, int seed, Tensor? seed_dev, int first_member, bool accumulate, Tensor? out_status=None, Tensor? out_sizes=None) -> int",
      &dietgpu_amd::decompress_data_update);
  m.def(
      "decompress_data_reduce(Tensor[] ts_in, int num_sources, Tensor[] ts_acc, int float_type, bool accumulate=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_sizes=None) -> int",
      &dietgpu_amd::decompress_data_reduce);
  m.def(
      "compress_data_cast(Tensor[] ts_in, int float_type, Tensor? temp_mem=None, Tensor? out_compressed=None, Tensor? out_compressed_sizes=None) -> (Tensor, Tensor, int)",
      &dietgpu_amd::compress_data_cast);
  m.def(
      "compress_data_feedback(Tensor[] ts_in, Tensor[] ts_residual, int float_type, bool fresh=False, Tensor? temp_mem=None, Tensor? out_compressed=None, Tensor? out_compressed_sizes=None) -> (Tensor, Tensor, int)",
      &dietgpu_amd::compress_data_feedback);
  m.def(
      "compress_data_stochastic(Tensor[] ts_in, int float_type, int seed, Tensor? seed_dev=None, int first_member=0, Tensor? out_compressed=None, Tensor? out_compressed_sizes=None) -> (Tensor, Tensor)",
      &dietgpu_amd::compress_data_stochastic);
  m.def(
      "compress_data_rolling(Tensor[] ts_in, Tensor? counts_in, Tensor? counts_out, int float_type, bool source_float32=False, Tensor? temp_mem=None, Tensor? out_compressed=None, Tensor? out_compressed_sizes=None) -> (Tensor, Tensor, int)",
      &dietgpu_amd::compress_data_rolling);
  m.def(
      "decompress_data_reduce_compress(Tensor[] ts_in, int num_sources, Tensor[] ts_acc, int float_type, bool accumulate=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_sizes=None, Tensor? out_compressed=None, Tensor? out_compressed_sizes=None) -> (Tensor, Tensor, int)",
      &dietgpu_amd::decompress_data_reduce_compress);
  m.def(
      "decompress_data_reduce_mixed(Tensor[] ts_in, int num_sources, Tensor[] ts_acc, int float_type, bool accumulate=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_sizes=None) -> int",
      &dietgpu_amd::decompress_data_reduce_mixed);
  m.def(
      "decompress_data_reduce_compress_mixed(Tensor[] ts_in, int num_sources, Tensor[] ts_acc, int float_type, bool accumulate=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_sizes=None, Tensor? out_compressed=None, Tensor? out_compressed_sizes=None) -> (Tensor, Tensor, int)",
      &dietgpu_amd::decompress_data_reduce_compress_mixed);
  m.def(
      "decompress_data_reduce_scaled(Tensor[] ts_in, int num_sources, Tensor[] ts_acc, int float_type, float scale, bool accumulate=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_sizes=None) -> int",
      &dietgpu_amd::decompress_data_reduce_scaled);
  m.def(
      "decompress_data_reduce_compress_scaled(Tensor[] ts_in, int num_sources, Tensor[] ts_acc, int float_type, float scale, bool accumulate=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_sizes=None, Tensor? out_compressed=None, Tensor? out_compressed_sizes=None) -> (Tensor, Tensor, int)",
      &dietgpu_amd::decompress_data_reduce_compress_scaled);
  m.def(
      "decompress_data_reduce_norm(Tensor[] ts_in, int num_sources, Tensor[] ts_acc, int float_type, float scale, bool accumulate=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_sizes=None, Tensor? out_sumsq=None, Tensor? out_nonfinite=None) -> int",
      &dietgpu_amd::decompress_data_reduce_norm);
  m.def(
      "decompress_data_reduce_compress_norm(Tensor[] ts_in, int num_sources, Tensor[] ts_acc, int float_type, float scale, bool accumulate=False, Tensor? temp_mem=None, Tensor? out_status=None, Tensor? out_sizes=None, Tensor? out_compressed=None, Tensor? out_compressed_sizes=None, Tensor? out_sumsq=None, Tensor? out_nonfinite=None) -> (Tensor, Tensor, int)",
      &dietgpu_amd::decompress_data_reduce_compress_norm);
}

TORCH_LIBRARY(dietgpu, m) {
  if (!coreLibraryMatches()) return;  // (the schemas above stay without implementations; ops.py does not use them)
  m.impl(TORCH_SELECTIVE_NAME("dietgpu::max_float_compressed_output_size"), TORCH_FN(dietgpu_amd::max_float_compressed_output_size));
  m.impl(TORCH_SELECTIVE_NAME("dietgpu::max_float_compressed_size"), TORCH_FN(dietgpu_amd::max_float_compressed_size));
  m.impl(TORCH_SELECTIVE_NAME("dietgpu::max_any_compressed_output_size"), TORCH_FN(dietgpu_amd::max_any_compressed_output_size));
  m.impl(TORCH_SELECTIVE_NAME("dietgpu::max_any_compressed_size"), TORCH_FN(dietgpu_amd::max_any_compressed_size));
  m.impl(TORCH_SELECTIVE_NAME("dietgpu::compress_data"), TORCH_FN(dietgpu_amd::compress_data));
  m.impl(TORCH_SELECTIVE_NAME("dietgpu::compress_data_split_size"), TORCH_FN(dietgpu_amd::compress_data_split_size));
  m.impl(TORCH_SELECTIVE_NAME("dietgpu::compress_data_simple"), TORCH_FN(dietgpu_amd::compress_data_simple));
  m.impl(TORCH_SELECTIVE_NAME("dietgpu::decompress_data"), TORCH_FN(dietgpu_amd::decompress_data));
  m.impl(TORCH_SELECTIVE_NAME("dietgpu::decompress_data_split_size"), TORCH_FN(dietgpu_amd::decompress_data_split_size));
  m.impl(TORCH_SELECTIVE_NAME("dietgpu::decompress_data_simple"), TORCH_FN(dietgpu_amd::decompress_data_simple));
  gOpsRegistered = true;
}
