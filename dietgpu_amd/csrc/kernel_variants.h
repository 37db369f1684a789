// Which template instantiation of a kernel a launch uses.  Every family's instantiations share one signature, so a
// launchable variant is a value: the kernel, its workgroup size, its dynamic LDS bytes and its profiling name.  The
// selection functions below are the only place where an instantiation is named and where "which forms exist" is
// stated; asking for a form that does not exist returns the nearest one that does.
#pragma once

#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <type_traits>

#include "format.h"
#include "kernels_decode.h"
#include "kernels_encode.h"
#include "kernels_pairs.h"
#include "kernels_stats.h"

namespace dgpu {

template <typename... Args>
struct KernelVariant {
  void (*fn)(Args...);
  uint32_t threads;   // workgroup size
  uint32_t ldsBytes;  // dynamic LDS
  const char* name;   // for DGPU_LAUNCH / dgpu_prof_summary
};
using EncodeVariant = KernelVariant<EncodeArgs>;
using DecodeVariant = KernelVariant<DecodeArgs>;
using HistogramVariant = KernelVariant<BatchView, uint32_t*, uint32_t, HistFuse>;
using StatsSingleVariant = KernelVariant<BatchView, NormalizeArgs, const uint32_t*, uint32_t>;

// Workgroups of `v` that fit on one CU at once (at least 1).  Asked of the runtime once per variant and process.
template <typename... Args>
uint32_t workgroupsPerCu(const KernelVariant<Args...>& v) {
  static std::mutex mu;
  static std::map<const void*, uint32_t> cache;
  std::lock_guard<std::mutex> g(mu);
  auto it = cache.find((const void*)v.fn);
  if (it != cache.end()) return it->second;
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, v.fn, (int)v.threads, v.ldsBytes) != hipSuccess || n < 1) n = 1;
  return cache[(const void*)v.fn] = (uint32_t)n;
}

// Run-time value -> compile-time constant: f receives a std::integral_constant.
template <uint32_t V>
using UintC = std::integral_constant<uint32_t, V>;
template <typename F>
auto withFloatType(uint32_t ft, F&& f) {
  switch (ft) {
    case 0: return f(UintC<0>{});
    case kFloat16: return f(UintC<kFloat16>{});
    case kBFloat16: return f(UintC<kBFloat16>{});
    default: return f(UintC<kFloat32>{});
  }
}
template <typename F>
auto withProbBits(int P, F&& f) {
  switch (P) {
    case 9: return f(std::integral_constant<int, 9>{});
    case 10: return f(std::integral_constant<int, 10>{});
    default: return f(std::integral_constant<int, 11>{});
  }
}
template <typename F>
auto withProbBitsAndFloatType(int P, uint32_t ft, F&& f) {
  return withFloatType(ft, [&](auto kFT) { return withProbBits(P, [&](auto kP) { return f(kP, kFT); }); });
}

// Float inputs use the small-stage / spilling encoder (6 workgroups per CU), raw bytes the worst-case stage (3 per
// CU; kernels_encode.h).
constexpr bool encodeSpills(uint32_t ft) { return ft != 0; }

// Cast sources (kCastSource: float32 words in, the archive of a 16-bit type out) exist as tiled encoders of 2, 4 and 8
// blocks in the dispatch forms of the plain 16-bit call -- 2- and 4-block tiles persistent and hardware-dispatched,
// 8-block tiles persistent -- without the wide stage, and as every histogram form.  There is no cast form of the
// single-block kernels (k_ans_encode_pair, k_stats_single): single-block members of a cast call run on 2-block tiles.
// Feedback sources (kFeedbackSource as well: the residual added before the rounding, the rounding error stored) exist
// in exactly the cast source's forms, and so do stochastic sources (kStochasticSource: every rounding stochastic).
// `extra`: 0, kFeedbackSource or kStochasticSource.
inline EncodeVariant encoderVariantCast(int P, uint32_t archiveType, uint32_t tileBlocks, bool hwDispatch, uint32_t extra = 0u) {
  auto of = [&](auto p, auto f) -> EncodeVariant {
    constexpr int kP = decltype(p)::value;
    constexpr uint32_t kFT = decltype(f)::value | kCastSource;
    auto tiled = [](auto tb, auto persistent) -> EncodeVariant {
      constexpr uint32_t kTB = decltype(tb)::value;
      constexpr bool kPersistent = decltype(persistent)::value;
      return {k_ans_encode<kP, kFT, true, kTB, kPersistent, false>, encThreads(kTB), encLdsBytes(kP, true, kFT, kTB),
              encIsStochastic(kFT) ? "k_ans_encode_stochastic" : (encIsFeedback(kFT) ? "k_ans_encode_feedback" : "k_ans_encode_cast")};
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (tileBlocks <= kBlocksPerTinyTile) return hwDispatch ? tiled(UintC<kBlocksPerTinyTile>{}, no) : tiled(UintC<kBlocksPerTinyTile>{}, yes);
    if (tileBlocks == kBlocksPerSmallTile) return hwDispatch ? tiled(UintC<kBlocksPerSmallTile>{}, no) : tiled(UintC<kBlocksPerSmallTile>{}, yes);
    return tiled(UintC<kBlocksPerTile>{}, yes);
  };
  return withProbBits(P, [&](auto p) {
    if (extra == kFeedbackSource) return archiveType == kFloat16 ? of(p, UintC<kFloat16 | kFeedbackSource>{}) : of(p, UintC<kBFloat16 | kFeedbackSource>{});
    if (extra == kStochasticSource) return archiveType == kFloat16 ? of(p, UintC<kFloat16 | kStochasticSource>{}) : of(p, UintC<kBFloat16 | kStochasticSource>{});
    return archiveType == kFloat16 ? of(p, UintC<kFloat16>{}) : of(p, UintC<kBFloat16>{});
  });
}

// The counting form (kernels_encode.h, kCount): persistent tiled encoders of 2, 4 and 8 blocks for float16 / bfloat16
// sources and their cast sources.  There is no hardware-dispatched, wide-stage or single-block form: single-block
// members run on 2-block tiles (the plan of a counting call has no single-block class, work_plan.h).
inline EncodeVariant encoderVariantCounting(int P, uint32_t ft, uint32_t tileBlocks) {
  auto of = [&](auto p, auto f) -> EncodeVariant {
    constexpr int kP = decltype(p)::value;
    constexpr uint32_t kFT = decltype(f)::value;
    auto tiled = [](auto tb) -> EncodeVariant {
      constexpr uint32_t kTB = decltype(tb)::value;
      return {k_ans_encode<kP, kFT, true, kTB, true, false, true>, encThreads(kTB), encCountLdsBytes(kP, kFT, kTB),
              encIsCast(kFT) ? "k_ans_encode_cast_count" : "k_ans_encode_count"};
    };
    if (tileBlocks <= kBlocksPerTinyTile) return tiled(UintC<kBlocksPerTinyTile>{});
    if (tileBlocks == kBlocksPerSmallTile) return tiled(UintC<kBlocksPerSmallTile>{});
    return tiled(UintC<kBlocksPerTile>{});
  };
  return withProbBits(P, [&](auto p) {
    if (encIsCast(ft)) return encArchiveType(ft) == kFloat16 ? of(p, UintC<kFloat16 | kCastSource>{}) : of(p, UintC<kBFloat16 | kCastSource>{});
    return encArchiveType(ft) == kFloat16 ? of(p, UintC<kFloat16>{}) : of(p, UintC<kBFloat16>{});
  });
}

// The encoder of tiles of `tileBlocks` blocks; ft: the archive's float type, with kCastSource for a cast source.
//   * single-block tiles go to k_ans_encode_pair: two ELEMENTS per wavefront, always one workgroup per pair;
//   * hwDispatch: one workgroup per tile, dispatched by the hardware in ticket order, instead of persistent workgroups
//     that walk the tickets.  8-block float tiles exist in the persistent form only (hardware dispatch measured no
//     gain there);
//   * wide: the wide stage (kSpillStageWordsWide) exists for persistent 8-block bf16 / fp32 tiles only.
inline EncodeVariant encoderVariant(int P, uint32_t ft, uint32_t tileBlocks, bool hwDispatch, bool wide) {
  if (encIsCast(ft)) return encoderVariantCast(P, encArchiveType(ft), tileBlocks, hwDispatch, ft & (kFeedbackSource | kStochasticSource));
  return withProbBitsAndFloatType(P, ft, [&](auto p, auto f) -> EncodeVariant {
    constexpr int kP = decltype(p)::value;
    constexpr uint32_t kFT = decltype(f)::value;
    constexpr bool kSpill = encodeSpills(kFT);
    if (tileBlocks == kBlocksPerSingleTile) {
      return {k_ans_encode_pair<kP, kFT, kSpill>, 64u, encPairLdsBytes(kP, kSpill, kFT), "k_ans_encode_pair"};
    }
    auto tiled = [](auto tb, auto persistent, auto wideStage) -> EncodeVariant {
      constexpr uint32_t kTB = decltype(tb)::value;
      constexpr bool kPersistent = decltype(persistent)::value, kWide = decltype(wideStage)::value;
      return {k_ans_encode<kP, kFT, kSpill, kTB, kPersistent, kWide>, encThreads(kTB), encLdsBytes(kP, kSpill, kFT, kTB, kWide),
              "k_ans_encode"};
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (tileBlocks == kBlocksPerTinyTile) {
      return hwDispatch ? tiled(UintC<kBlocksPerTinyTile>{}, no, no) : tiled(UintC<kBlocksPerTinyTile>{}, yes, no);
    }
    if (tileBlocks == kBlocksPerSmallTile) {
      return hwDispatch ? tiled(UintC<kBlocksPerSmallTile>{}, no, no) : tiled(UintC<kBlocksPerSmallTile>{}, yes, no);
    }
    if constexpr (kFT == kBFloat16 || kFT == kFloat32) {
      if (wide) return tiled(UintC<kBlocksPerTile>{}, yes, yes);
    }
    if constexpr (!kSpill) {
      if (hwDispatch) return tiled(UintC<kBlocksPerTile>{}, no, no);
    }
    return tiled(UintC<kBlocksPerTile>{}, yes, no);
  });
}

// The archive type a decode form is built for, given the call's.
constexpr uint32_t sameType(uint32_t ft) { return ft; }
constexpr uint32_t floatsOnly(uint32_t ft) { return ft ? ft : kFloat32; }                         // raw bytes: the float32 form
constexpr uint32_t halvesOnly(uint32_t ft) { return ft == kFloat16 ? kFloat16 : kBFloat16; }  // anything but fp16: the bf16 form

// Every decode form but the whole decode, once: X(form, kernel template, archive-type substitution, LDS bytes of the
// instantiation <P, T, TB>).  The kernel's name is its profiling name.  Each exists for 16- and 4-block tiles; a new
// form is one line here.
//   * kAccum: widens to float32 and stores to / adds into float32 accumulators; float types only;
//   * kReduce: the same with DecodeArgs::numSources archives per accumulator;
//   * kReduceStats: also counts the exponent bytes of the rounded sums (DecodeArgs::stats); float16 and bfloat16 only,
//     with the LDS of the bins behind that of the plain form;
//   * kReduceMixed / kReduceMixedStats: the two above with sources that are archives or raw rows (DecodeArgs::sourceKind);
//     the same types, tiles and LDS;
//   * kReduceScaled / kReduceScaledStats: the mixed forms that multiply the last source's store by DecodeArgs::scale;
//     they serve all-archive members too.  The counting form keeps the factor in LDS behind its bins;
//   * kReduceNorm / kReduceNormStats: the scaled forms that also measure the words they leave (DecodeArgs::normPartials)
//     and take a factor of 1 as well; the LDS of the scaled forms and a ReduceNormTile behind it;
//   * kWholeScaled: the whole decode that multiplies every word by the member's factor (DecodeArgs::scalePtr /
//     scaleStride / scale); float types only, the LDS of the whole form.  There is no scaled form of k_ans_decode_pair:
//     single-block batches run on 4-block tiles;
//   * kAccumScaled: kAccum whose widened word is multiplied by the member's factor (as kWholeScaled takes it) before
//     the store or the add; float types only, the LDS of kAccum;
//   * kUpdate: kAccumScaled into 16-bit tensors of the archive's type, rounded stochastically (DecodeArgs::seedPtr /
//     seed / firstMember); float16 and bfloat16 only, the LDS of kAccum;
//   * kRanged: decodes a block range of every element (a range of one or two blocks takes the 4-block form).
#define DGPU_DECODE_FORMS(X)                                                                                           \
  X(kAccum, k_ans_decode_accum, floatsOnly, decLdsBytes(P, T, TB))                                                     \
  X(kReduce, k_ans_decode_reduce, floatsOnly, decLdsBytes(P, T, TB))                                                   \
  X(kReduceStats, k_ans_decode_reduce_stats, halvesOnly, decReduceStatsLdsBytes(P, T, TB))                             \
  X(kReduceMixed, k_ans_decode_reduce_mixed, floatsOnly, decLdsBytes(P, T, TB))                                        \
  X(kReduceMixedStats, k_ans_decode_reduce_mixed_stats, halvesOnly, decReduceStatsLdsBytes(P, T, TB))                  \
  X(kReduceScaled, k_ans_decode_reduce_mixed_scaled, floatsOnly, decLdsBytes(P, T, TB))                                \
  X(kReduceScaledStats, k_ans_decode_reduce_mixed_stats_scaled, halvesOnly, decReduceStatsScaledLdsBytes(P, T, TB))    \
  X(kReduceNorm, k_ans_decode_reduce_mixed_norm, floatsOnly, decReduceNormLdsBytes(P, T, TB, false))                   \
  X(kReduceNormStats, k_ans_decode_reduce_mixed_stats_norm, halvesOnly, decReduceNormLdsBytes(P, T, TB, true))         \
  X(kWholeScaled, k_ans_decode_scaled, floatsOnly, decScaledLdsBytes(P, T, TB))                                        \
  X(kAccumScaled, k_ans_decode_accum_scaled, floatsOnly, decLdsBytes(P, T, TB))                                        \
  X(kUpdate, k_ans_decode_update, halvesOnly, decLdsBytes(P, T, TB))                                                   \
  X(kRanged, k_ans_decode_range, sameType, decLdsBytes(P, T, TB))

// The decoder of tiles of `tileBlocks` blocks.  A form of the list above takes the 4-block instantiation for tiles of
// up to 4 blocks and the 16-block one otherwise.  The whole decode (k_ans_decode) also exists for 2-block tiles, and
// batches whose every capacity is one block go to k_ans_decode_pair (two elements per wavefront, kernels_pairs.h).
inline DecodeVariant decoderVariant(int P, uint32_t ft, uint32_t tileBlocks, DecodeForm form = DecodeForm::kWhole) {
  return withProbBitsAndFloatType(P, ft, [&](auto p, auto f) -> DecodeVariant {
    constexpr int kP = decltype(p)::value;
    constexpr uint32_t kFT = decltype(f)::value;
    auto smallOrFull = [&](auto tiled) -> DecodeVariant {
      return tileBlocks <= kDecBlocksPerSmallTile ? tiled(UintC<kDecBlocksPerSmallTile>{}) : tiled(UintC<kDecBlocksPerTile>{});
    };
#define DGPU_DECODE_FORM_CASE(formName, kernel, typeOf, ldsBytes)                \
  if (form == DecodeForm::formName) {                                            \
    return smallOrFull([](auto tb) -> DecodeVariant {                            \
      constexpr int P = kP;                                                      \
      constexpr uint32_t T = typeOf(kFT), TB = decltype(tb)::value;              \
      return {kernel<P, T, TB>, decThreads(TB), ldsBytes, #kernel};              \
    });                                                                          \
  }
    DGPU_DECODE_FORMS(DGPU_DECODE_FORM_CASE)
#undef DGPU_DECODE_FORM_CASE
    if (tileBlocks == kDecBlocksPerSingleTile) return {k_ans_decode_pair<kP, kFT>, 64u, decPairLdsBytes(kP, kFT), "k_ans_decode_pair"};
    auto tiled = [](auto tb) -> DecodeVariant {
      constexpr uint32_t kTB = decltype(tb)::value;
      return {k_ans_decode<kP, kFT, kTB>, decThreads(kTB), decLdsBytes(kP, kFT, kTB), "k_ans_decode"};
    };
    if (tileBlocks == kDecBlocksPerTinyTile) return tiled(UintC<kDecBlocksPerTinyTile>{});
    if (tileBlocks == kDecBlocksPerSmallTile) return tiled(UintC<kDecBlocksPerSmallTile>{});
    return tiled(UintC<kDecBlocksPerTile>{});
  });
}

// The histogram pass: bins with kHistSlotsSmall or kHistSlotsLarge lane slots, non-temporal or ordinary input loads.
// (ft with kCastSource: the cast form, which bins the exponent byte of the rounded word; with kFeedbackSource or
// kStochasticSource as well: that source's rounding)
inline HistogramVariant histogramVariant(uint32_t ft, bool smallBins, bool nonTemporal) {
  auto pick = [&](auto f) -> HistogramVariant {
    constexpr uint32_t kFT = decltype(f)::value;
    auto of = [](auto slots, auto nt) -> HistogramVariant {
      constexpr uint32_t kS = decltype(slots)::value;
      constexpr bool kNt = decltype(nt)::value;
      if constexpr (kFT == 0) {
        return {k_histogram<kS, kNt>, 256u, 0u, "k_histogram"};
      } else {
        return {k_float_histogram<kFT, kS, kNt>, 256u, 0u,
                encIsStochastic(kFT) ? "k_float_histogram_stochastic"
                                     : (encIsFeedback(kFT) ? "k_float_histogram_feedback" : (encIsCast(kFT) ? "k_float_histogram_cast" : "k_float_histogram"))};
      }
    };
    constexpr UintC<kHistSlotsSmall> small{};
    constexpr UintC<kHistSlotsLarge> large{};
    if (nonTemporal) return smallBins ? of(small, std::true_type{}) : of(large, std::true_type{});
    return smallBins ? of(small, std::false_type{}) : of(large, std::false_type{});
  };
  if (encIsFeedback(ft)) {
    return encArchiveType(ft) == kFloat16 ? pick(UintC<kFloat16 | kCastSource | kFeedbackSource>{}) : pick(UintC<kBFloat16 | kCastSource | kFeedbackSource>{});
  }
  if (encIsStochastic(ft)) {
    return encArchiveType(ft) == kFloat16 ? pick(UintC<kFloat16 | kCastSource | kStochasticSource>{}) : pick(UintC<kBFloat16 | kCastSource | kStochasticSource>{});
  }
  if (encIsCast(ft)) return encArchiveType(ft) == kFloat16 ? pick(UintC<kFloat16 | kCastSource>{}) : pick(UintC<kBFloat16 | kCastSource>{});
  return withFloatType(ft, pick);
}

// One wavefront counts and normalises a single-block element (kernels_pairs.h).  Not built for float32, whose batches
// keep the workgroup per element (encodeCommon).
inline StatsSingleVariant statsSingleVariant(uint32_t ft, bool nonTemporal) {
  return withFloatType(ft, [&](auto f) -> StatsSingleVariant {
    constexpr uint32_t kFT = decltype(f)::value == kFloat32 ? kBFloat16 : decltype(f)::value;
    if (nonTemporal) return {k_stats_single<kFT, true>, 64u * kSingleStatWaves, 0u, "k_stats_single"};
    return {k_stats_single<kFT, false>, 64u * kSingleStatWaves, 0u, "k_stats_single"};
  });
}

}  // namespace dgpu
