// What the kernels and the host's work planning (work_plan.h) both go by: block size, float types, tile geometries.
// Includes nothing but <stdint.h>, so the planner and its test program compile without ROCm.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define DGPU_HD __host__ __device__
#else
#define DGPU_HD
#endif

namespace dgpu {

constexpr uint32_t kBlockSize = 4096;  // kDefaultBlockSize, GpuANSUtils.cuh:37
constexpr uint32_t kFloat16 = 1, kBFloat16 = 2, kFloat32 = 3;

DGPU_HD constexpr uint32_t divUp(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
DGPU_HD constexpr uint32_t roundUp(uint32_t a, uint32_t b) { return divUp(a, b) * b; }
DGPU_HD inline uint32_t floatWordBytes(uint32_t ft) { return ft == kFloat32 ? 4u : 2u; }

// SOURCE of an encoder / histogram instantiation: the template parameter FT is the archive's float type, or -- cast
// sources, which read float32 words and round them to the archive's 16-bit type in registers -- that type with
// kCastSource set.  Everything about the ARCHIVE (layout, header, stage size) goes by encArchiveType(FT).
constexpr uint32_t kCastSource = 0x100u;
DGPU_HD constexpr bool encIsCast(uint32_t ft) { return (ft & kCastSource) != 0u; }
// kCountingSource (a PLANNING flag only, never a template parameter): the call runs the counting form of the encoder
// (kernels_encode.h, kCount), which like the cast sources exists as tiles of 2, 4 and 8 blocks only.
constexpr uint32_t kCountingSource = 0x200u;
// kFeedbackSource (with kCastSource): a cast source with error feedback -- a float32 residual per word is added before
// the rounding and the new rounding error stored back (kernels_encode.h, ChunkSourceFeedback).  Planned and launched as
// the cast source it extends; there is no counting form.
constexpr uint32_t kFeedbackSource = 0x400u;
DGPU_HD constexpr bool encIsFeedback(uint32_t ft) { return (ft & kFeedbackSource) != 0u; }
// kStochasticSource (with kCastSource): a cast source that rounds stochastically, with random bits that are a pure
// function of (seed, member, word index within the element) -- the histogram and the encoder round the same word in
// different kernels and must agree (kernels_encode.h, ChunkSourceStochastic).  Planned and launched as the cast source;
// there is no counting and no feedback form.
constexpr uint32_t kStochasticSource = 0x800u;
DGPU_HD constexpr bool encIsStochastic(uint32_t ft) { return (ft & kStochasticSource) != 0u; }
DGPU_HD constexpr uint32_t encArchiveType(uint32_t ft) { return ft & ~(kCastSource | kCountingSource | kFeedbackSource | kStochasticSource); }
// whether single-block elements of such a call have kernels of their own (k_ans_encode_pair, k_stats_single)
DGPU_HD constexpr bool encHasSingleBlockKernels(uint32_t ft) { return (ft & (kCastSource | kCountingSource)) == 0u && ft != kFloat32; }

// Encoder: blocks per tile = per workgroup.  8 (256 threads: 4 wave64 x 2 half-waves); 4 (128 threads) for batches whose
// elements have at most 4 blocks -- an 8-block tile would leave half of its waves without a block there; a single
// wavefront for batches of elements of at most 2 blocks: half the LDS per workgroup, twice the resident tiles; batches
// of SINGLE-block elements go to k_ans_encode_pair (kernels_pairs.h): two ELEMENTS per wavefront.
constexpr uint32_t kBlocksPerTile = 8, kBlocksPerSmallTile = 4, kBlocksPerTinyTile = 2, kBlocksPerSingleTile = 1;

// Decoder: a workgroup is 8 wavefronts = 16 blocks sharing one LUT: 32 KiB of rings + 8 KiB LUT (P = 10) lets 4
// workgroups = 32 wavefronts (the maximum) reside on a CU.  Batches of small elements (a few blocks each) use 4-block
// workgroups instead: a 16-block workgroup would leave most of its waves without a block while still holding its LDS
// and wave slots; one wavefront per element for batches of elements of at most 2 blocks; batches of single-block
// elements (every capacity <= 4096 symbols) go to k_ans_decode_pair (kernels_pairs.h): two ELEMENTS per wavefront.
constexpr uint32_t kDecBlocksPerTile = 16, kDecBlocksPerSmallTile = 4, kDecBlocksPerTinyTile = 2, kDecBlocksPerSingleTile = 1;

}  // namespace dgpu
