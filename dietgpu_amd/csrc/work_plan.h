// Work planning: what a call launches, from the sizes of its batch -- tile geometry, the work lists of ragged batches,
// size classes, histogram parts, the plan cache.  Pure host arithmetic: no HIP, no globals (the test hooks of capi.hip
// arrive as PlanPolicy), so tests/cpp/plan_dump.cpp exercises it on the CPU.
//
// A plan is a non-empty vector of LaunchGroups, launched one after the other, plus the `work` vector their lists live
// in (Batch::work, uploaded with the pointers):
//   * a rectangle call: one unlisted group -- the grid is laid out for the LARGEST element, as upstream's is;
//   * a ragged batch: one listed group -- the whole batch on one geometry, only the work that exists;
//   * a batch split into size classes: several listed groups, each on its own geometry, large elements first.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <iterator>
#include <map>
#include <vector>

#include "plan_constants.h"

namespace dgpu {

// dgpu_debug_set_work_lists / dgpu_debug_set_size_classes: -1 = the policies below, 0 = off, 1 = wherever possible
struct PlanPolicy { int workLists = -1, sizeClasses = -1; };

// Lists are words of `work`: tiles and histogram parts as element << 16 | tile or part, tile bases and elements plain.
struct LaunchGroup {
  uint32_t tileBlocks = 0;
  uint32_t maxSize = 0;   // the group's largest element: symbols (encode), blocks (decode)
  uint32_t maxTiles = 0;  // ... and its tiles
  bool listed = false;    // false: the rectangle [numInBatch] x [maxTiles], nothing in `work`
  uint32_t tilesAt = 0, numTiles = 0;                        // tiles of >= 2 blocks: [numTiles]
  uint32_t histAt = 0, numHistParts = 0, histPartBytes = 0;  // encode without a caller's histogram: [numHistParts]
  uint32_t tileBaseAt = 0;                                   // encode: [numInBatch] first ticket of each of the group's elements
  uint32_t elemsAt = 0, numElems = 0;                        // single-block class: [numElems] the elements to pair up
};

// ---- Geometry ----
// blocks per encoder tile for a batch whose largest element has `maxSize` symbols; ft: what is encoded (0: raw bytes; a
// float type, with kCastSource for a cast call or kCountingSource for a counting one, which have no single-block
// kernels: their single-block elements run on 2-block tiles)
inline uint32_t encTileBlocksFor(uint32_t maxSize, uint32_t ft = 0) {
  const uint32_t blocks = divUp(maxSize, kBlockSize);
  if ((ft & (kCastSource | kCountingSource)) != 0u && blocks <= kBlocksPerTinyTile) return kBlocksPerTinyTile;
  return blocks <= kBlocksPerSingleTile ? kBlocksPerSingleTile
      : blocks <= kBlocksPerTinyTile    ? kBlocksPerTinyTile
      : blocks <= kBlocksPerSmallTile   ? kBlocksPerSmallTile
                                        : kBlocksPerTile;
}
inline uint32_t tilesFor(uint32_t maxSize, uint32_t ft = 0) { return divUp(divUp(maxSize, kBlockSize), encTileBlocksFor(maxSize, ft)); }

// blocks per decoder tile for a batch whose largest capacity has `maxBlocks` blocks: elements of up to 8 blocks:
// 4-block workgroups, of up to 2 blocks: one wavefront (see kDecBlocksPerSmallTile).  The ranged and the accumulating
// form (!whole) exist for two geometries only.
inline uint32_t decTileBlocksFor(uint32_t maxBlocks, bool whole = true) {
  if (!whole) return maxBlocks <= 2u * kDecBlocksPerSmallTile ? kDecBlocksPerSmallTile : kDecBlocksPerTile;
  return maxBlocks <= 1u ? kDecBlocksPerSingleTile
      : maxBlocks <= 2u  ? kDecBlocksPerTinyTile
      : maxBlocks <= 8u  ? kDecBlocksPerSmallTile
                         : kDecBlocksPerTile;
}

inline LaunchGroup encodeRectangle(uint32_t maxSize, uint32_t ft) { return {encTileBlocksFor(maxSize, ft), maxSize, tilesFor(maxSize, ft)}; }
inline LaunchGroup decodeRectangle(uint32_t maxBlocks, bool whole) {
  const uint32_t tileBlocks = decTileBlocksFor(maxBlocks, whole);
  return {tileBlocks, maxBlocks, std::max(1u, divUp(maxBlocks, tileBlocks))};
}

// ---- Lists ----
// Batches whose elements differ widely in size -- the tensors of a model in one call: a few matrices, many vectors.
// With one 32 Mi-word tensor next to 255 small ones the rectangle is 262 144 encoder tickets of which 1 279
// exist, spread over the persistent workgroups by a static map that hands the large tensor's tiles to three of them,
// and two histogram workgroups for its 64 MiB (tools/ragged_probe.py: 5.7 ms per compress call against 56 us + 37 us
// for the two size classes on their own).  The host knows the sizes (they arrive as host arrays), so for such a batch
// it lists the work that exists and the kernels take their (element, tile / part) from the list:
//   * tiles: the encoder's element by element, the large elements first (a tile's predecessor has the ticket before
//     its own, and descriptors and claim words exist for the listed tiles only); the decoder's, which do not depend on
//     one another, tile-major;
//   * histogram parts: every element cut into parts of histPartBytes (chosen for the usual number of workgroups over
//     the WHOLE batch or class), element-major, so that an element's partial histograms are consecutive.
// Used when at least a fifth of the rectangle's tiles do not exist (256 bf16 tensors of 0.06 .. 1 Mi words: compress
// 228 -> 181 us; of 0.5 .. 1 Mi: 247 -> 229; of 0.85 .. 1 Mi the rectangle is 3 % faster: profiles/r05_ab_work_lists.txt).
inline uint64_t divUp64(uint64_t a, uint64_t b) { return (a + b - 1u) / b; }
inline uint64_t roundUp64(uint64_t a, uint64_t b) { return divUp64(a, b) * b; }

// Whether the tiles (of `tileSymbols` symbols) of a batch on one geometry are listed; then *tiles holds every element's
// count and *order the elements by descending count.  minTiles: 1 where an element without symbols still needs its
// first tile (decode).  mode: PlanPolicy::workLists, or 1 for ranged decode, which has no rectangle to fall back to.
inline bool raggedOrder(int mode, const std::vector<uint32_t>& sizes, uint32_t tileSymbols, uint32_t maxTiles, uint32_t minTiles,
                        std::vector<uint32_t>* tiles, std::vector<uint32_t>* order, std::vector<uint32_t>* work) {
  const size_t B = sizes.size();
  if (mode == 0 || B == 0 || B > 65535u || maxTiles > 65536u || tileSymbols == 0) return false;
  tiles->resize(B);
  uint64_t total = 0;
  for (size_t b = 0; b < B; ++b) {
    (*tiles)[b] = std::max(divUp(sizes[b], tileSymbols), minTiles);
    total += (*tiles)[b];
  }
  if (mode != 1 && (B < 2 || maxTiles < 2 || total * 5u > (uint64_t)B * maxTiles * 4u)) return false;
  if (total > 0x7fffffffull) return false;
  order->resize(B);
  for (size_t b = 0; b < B; ++b) (*order)[b] = (uint32_t)b;
  std::stable_sort(order->begin(), order->end(), [&](uint32_t x, uint32_t y) { return (*tiles)[x] > (*tiles)[y]; });
  work->reserve(work->size() + (size_t)total);
  return true;
}
// Element-major (encoder): the tiles of each of `elems` are consecutive -- descriptors and claim words are then indexed
// by the ticket; tileBase[b] receives the first ticket of element b.  tiles[]: by element.
inline void listTilesElementMajor(const std::vector<uint32_t>& elems, const std::vector<uint32_t>& tiles, std::vector<uint32_t>* tileBase,
                                  std::vector<uint32_t>* work) {
  const size_t first = work->size();
  tileBase->assign(tiles.size(), 0u);
  for (uint32_t b : elems) {
    (*tileBase)[b] = (uint32_t)(work->size() - first);
    for (uint32_t r = 0; r < tiles[b]; ++r) work->push_back((b << 16) | r);
  }
}
// Tile-major (decoder); `elems` in descending tile count.
inline void listTilesTileMajor(const std::vector<uint32_t>& elems, const std::vector<uint32_t>& tiles, uint32_t maxTiles, std::vector<uint32_t>* work) {
  for (uint32_t r = 0; r < maxTiles; ++r)
    for (size_t i = 0; i < elems.size() && tiles[elems[i]] > r; ++i) work->push_back((elems[i] << 16) | r);
}
// Histogram parts of n elements (elems, or 0 .. n - 1 without it), sized for the usual number of workgroups over them
// (the classes of a call run one after the other, each should fill the chip).  wordBytes: of the archive's words, also
// for a cast call.  false: an element has more parts than a list entry can name.
constexpr uint32_t kHistTargetWgsForLists = 512, kHistTargetWgsForListsRaw = 768;
inline bool listHistParts(const uint32_t* elems, size_t n, const std::vector<uint32_t>& sizes, uint32_t wordBytes, bool raw, LaunchGroup* g,
                          std::vector<uint32_t>* work) {
  uint64_t totalBytes = 0;
  for (size_t i = 0; i < n; ++i) totalBytes += (uint64_t)sizes[elems ? elems[i] : i] * wordBytes;
  const uint64_t target = raw ? kHistTargetWgsForListsRaw : kHistTargetWgsForLists;
  const uint64_t partBytes = std::max<uint64_t>(32u * 1024u, roundUp64(divUp64(totalBytes, target), 16u * 1024u));
  g->histPartBytes = (uint32_t)std::min<uint64_t>(partBytes, 0x40000000ull);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t b = elems ? elems[i] : (uint32_t)i;
    const uint32_t parts = (uint32_t)std::max<uint64_t>(1u, divUp64((uint64_t)sizes[b] * wordBytes, g->histPartBytes));
    if (parts > 65536u) return false;
    for (uint32_t p = 0; p < parts; ++p) work->push_back((b << 16) | p);
  }
  g->numHistParts = (uint32_t)(work->size() - g->histAt);
  return true;
}
// The lists of an encode group: tiles of `elems` in that order, histogram parts (of the same elements in that order, or
// -- histInIndexOrder -- of the whole batch), tile bases.  ft: as encTileBlocksFor's.
inline bool listEncodeGroup(const std::vector<uint32_t>& elems, bool histInIndexOrder, const std::vector<uint32_t>& sizes,
                            const std::vector<uint32_t>& tiles, uint32_t ft, bool needHist, LaunchGroup* g, std::vector<uint32_t>* work) {
  std::vector<uint32_t> tileBase;
  g->listed = true;
  g->tilesAt = (uint32_t)work->size();
  listTilesElementMajor(elems, tiles, &tileBase, work);
  g->numTiles = (uint32_t)(work->size() - g->tilesAt);
  g->histAt = (uint32_t)work->size();
  const uint32_t wordBytes = ft ? floatWordBytes(encArchiveType(ft)) : 1u;
  if (needHist && !listHistParts(histInIndexOrder ? nullptr : elems.data(), elems.size(), sizes, wordBytes, ft == 0, g, work)) return false;
  g->tileBaseAt = (uint32_t)work->size();
  work->insert(work->end(), tileBase.begin(), tileBase.end());
  return true;
}

// ---- Size classes ----
// SIZE CLASSES inside one batch.  The tile geometry of a call -- pairs of single-block elements per wavefront, tiles of 2,
// 4 or 8 blocks -- used to be chosen once, from the largest element (upstream does the same: one grid laid out for
// maxSize, GpuANSEncode.cuh:753-771).  One large tensor next to thousands of small ones then ran every small element on
// an 8-block tile -- seven of its eight half-waves idle, where the pair kernels are 1.4-2 x faster on such elements.
// The host lists the work of such a batch PER CLASS and launches each class on the kernels of its own geometry, the
// classes one after the other on the caller's stream (large elements first).  All kernels index the batch's arrays by
// the element's own index, so a class is nothing but its lists: tiles and histogram parts or, for the single-block
// class, the elements to pair up.
// A class of fewer than kMinClassElements elements joins the next larger one (a launch costs more than their idle
// lanes), and a batch whose smaller classes together hold fewer than kMinSplitElements elements is not split at all:
// in ONE launch its few small elements run beside the large ones' tiles (1 x 32 Mi + 255 x 2 Ki bf16: 71 us together
// against 56 + 38 one after the other, profiles/r05_ab_work_lists.txt).
constexpr uint32_t kMinClassElements = 32, kMinSplitElements = 256;
// Splits the batch into size classes (false: one geometry for the call).  `classOf(size)` -> blocks per tile /
// workgroup of an element of that size; `pairsOk`: the single-block class has kernels of its own.
template <typename ClassOf>
bool classifyBySize(const PlanPolicy& policy, const std::vector<uint32_t>& sizes, ClassOf classOf, bool pairsOk,
                    std::vector<uint32_t>* classOfElem, std::vector<uint32_t>* classesOut) {
  const int mode = policy.sizeClasses;
  const size_t B = sizes.size();
  if (mode == 0 || policy.workLists == 0 || B < 2 || B > 65535u) return false;
  std::map<uint32_t, uint32_t> count;
  classOfElem->resize(B);
  for (size_t b = 0; b < B; ++b) {
    uint32_t c = classOf(sizes[b]);
    if (c == 1u && !pairsOk) c = 2u;
    (*classOfElem)[b] = c;
    count[c]++;
  }
  if (count.size() < 2) return false;
  // small classes join the next larger one that exists
  for (auto it = count.begin(); it != count.end();) {
    auto next = std::next(it);
    if (next != count.end() && it->second < (mode == 1 ? 1u : kMinClassElements)) {
      for (size_t b = 0; b < B; ++b) {
        if ((*classOfElem)[b] == it->first) (*classOfElem)[b] = next->first;
      }
      next->second += it->second;
      it = count.erase(it);
    } else {
      it = next;
    }
  }
  if (count.size() < 2) return false;
  uint32_t small = 0;
  for (auto& kv : count) {
    if (kv.first != count.rbegin()->first) small += kv.second;
  }
  if (mode != 1 && small < kMinSplitElements) return false;
  classesOut->clear();
  for (auto it = count.rbegin(); it != count.rend(); ++it) classesOut->push_back(it->first);  // large elements first
  return true;
}
// One listed group per class.  encode: element-major tiles, histogram parts and tile bases, nothing for an element
// without symbols; otherwise (decode, from the output capacities) tile-major tiles, one also for such an element.
// false, with `work` empty again: no split, or a class with an element of more tiles or parts than a list entry can name.
template <typename ClassOf>
bool planClasses(const PlanPolicy& policy, const std::vector<uint32_t>& sizes, ClassOf classOf, bool pairsOk, bool encode, uint32_t ft,
                 std::vector<LaunchGroup>* groups, std::vector<uint32_t>* work) {
  std::vector<uint32_t> classOfElem, order;
  if (!classifyBySize(policy, sizes, classOf, pairsOk, &classOfElem, &order)) return false;
  const size_t B = sizes.size();
  std::vector<uint32_t> tiles(B, 0u);
  groups->clear();
  for (uint32_t c : order) {
    LaunchGroup g;
    g.tileBlocks = c;
    g.listed = true;
    std::vector<uint32_t> elems;
    uint32_t maxSize = 0;
    for (size_t b = 0; b < B; ++b) {
      if (classOfElem[b] == c) {
        elems.push_back((uint32_t)b);
        maxSize = std::max(maxSize, sizes[b]);
      }
    }
    g.maxSize = encode ? maxSize : divUp(maxSize, kBlockSize);
    g.maxTiles = std::max(1u, divUp(divUp(maxSize, kBlockSize), c));
    bool ok = g.maxTiles <= 65536u;
    if (c == 1u) {
      g.elemsAt = (uint32_t)work->size();
      g.numElems = (uint32_t)elems.size();
      work->insert(work->end(), elems.begin(), elems.end());
    } else if (ok) {
      // the class's larger elements first
      std::stable_sort(elems.begin(), elems.end(), [&](uint32_t x, uint32_t y) { return sizes[x] > sizes[y]; });
      for (uint32_t b : elems) tiles[b] = std::max(divUp(sizes[b], c * kBlockSize), encode ? 0u : 1u);
      if (encode) {
        ok = listEncodeGroup(elems, false, sizes, tiles, ft, true, &g, work);
      } else {
        g.tilesAt = (uint32_t)work->size();
        listTilesTileMajor(elems, tiles, g.maxTiles, work);
        g.numTiles = (uint32_t)(work->size() - g.tilesAt);
      }
    }
    if (!ok) return work->clear(), groups->clear(), false;
    groups->push_back(g);
  }
  return true;
}

// A training or collective loop compresses the same list of tensors step after step: the last class plan of each kind is
// kept per host thread and reused when the sizes (and everything else the plan depends on) are the same -- planning a
// batch of 32 769 tensors costs ~100 us of host time, comparing its sizes 10.  `plan(groups, work)`: the planner; one
// cache per planner type, so one per direction.
struct ClassPlanCache {
  std::vector<uint32_t> sizes, work;
  std::vector<LaunchGroup> groups;
  uint32_t floatType = 0;
  PlanPolicy policy;
  bool valid = false, split = false;
};
template <typename Plan>
bool planClassesCached(const PlanPolicy& policy, const std::vector<uint32_t>& sizes, uint32_t ft, Plan plan, std::vector<LaunchGroup>* groups,
                       std::vector<uint32_t>* work) {
  if (sizes.size() < kMinSplitElements) return plan(groups, work);  // (cheap to plan, and rarely split)
  static thread_local ClassPlanCache cache;
  const bool hit = cache.valid && cache.floatType == ft && cache.policy.sizeClasses == policy.sizeClasses &&
      cache.policy.workLists == policy.workLists && cache.sizes.size() == sizes.size() &&
      memcmp(cache.sizes.data(), sizes.data(), sizes.size() * 4u) == 0;
  if (!hit) {
    cache.groups.clear(), cache.work.clear();
    cache.split = plan(&cache.groups, &cache.work);
    cache.sizes = sizes, cache.floatType = ft, cache.policy = policy, cache.valid = true;
  }
  if (!cache.split) return false;
  *groups = cache.groups;
  *work = cache.work;
  return true;
}

// ---- The plans of the calls.  `work` arrives empty. ----
// ft: as encTileBlocksFor's; a call with a caller's histogram is never split into classes and lists no histogram parts.
inline void planEncodeCall(const PlanPolicy& policy, const std::vector<uint32_t>& sizes, uint32_t ft, uint32_t maxSize, bool callerHist,
                           std::vector<LaunchGroup>* groups, std::vector<uint32_t>* work) {
  // (cast calls, counting calls and float32 have no single-block kernels)
  auto classes = [&](std::vector<LaunchGroup>* gr, std::vector<uint32_t>* wk) {
    return planClasses(policy, sizes, [](uint32_t sz) { return encTileBlocksFor(sz); }, encHasSingleBlockKernels(ft), true, ft, gr, wk);
  };
  if (!callerHist && planClassesCached(policy, sizes, ft, classes, groups, work)) return;
  LaunchGroup g = encodeRectangle(maxSize, ft);
  std::vector<uint32_t> tiles, order;
  // (single-block batches: one wavefront per element, nothing to list)
  if (g.tileBlocks != kBlocksPerSingleTile && raggedOrder(policy.workLists, sizes, g.tileBlocks * kBlockSize, g.maxTiles, 0u, &tiles, &order, work) &&
      !listEncodeGroup(order, true, sizes, tiles, ft, !callerHist, &g, work)) {
    work->clear();
    g = encodeRectangle(maxSize, ft);
  }
  groups->assign(1, g);
}

// whole: dgpu_*_decode_*; otherwise decode-accumulate, which runs on one geometry
inline void planDecodeCall(const PlanPolicy& policy, const std::vector<uint32_t>& caps, uint32_t maxCapacity, bool whole,
                           std::vector<LaunchGroup>* groups, std::vector<uint32_t>* work) {
  auto classes = [&](std::vector<LaunchGroup>* gr, std::vector<uint32_t>* wk) {
    return planClasses(policy, caps, [](uint32_t cap) { return decTileBlocksFor(divUp(cap, kBlockSize)); }, true, false, 0u, gr, wk);
  };
  if (whole && planClassesCached(policy, caps, 0u, classes, groups, work)) return;
  LaunchGroup g = decodeRectangle(divUp(maxCapacity, kBlockSize), whole);
  std::vector<uint32_t> tiles, order;
  // (capacities that differ widely: only the tiles inside each element's capacity are launched)
  if (g.tileBlocks != kDecBlocksPerSingleTile && raggedOrder(policy.workLists, caps, g.tileBlocks * kBlockSize, g.maxTiles, 1u, &tiles, &order, work)) {
    g.listed = true;
    g.tilesAt = (uint32_t)work->size();
    listTilesTileMajor(order, tiles, g.maxTiles, work);
    g.numTiles = (uint32_t)(work->size() - g.tilesAt);
  }
  groups->assign(1, g);
}

// Ranged decode: blocks [firstBlock[i], firstBlock[i] + numBlocks[i]) of every element.  One geometry per call, chosen
// from the largest range; firstBlock[B] and numBlocks[B] travel in front of the list, which holds the tiles of each
// range, counted from its first block: as many as the request and the capacity allow.  false: too many tiles for a call.
inline bool planRangeCall(uint32_t B, const uint32_t* firstBlock, const uint32_t* numBlocks, const uint32_t* outCapacity, LaunchGroup* group,
                          std::vector<uint32_t>* work) {
  std::vector<uint32_t> rangeSymbols(B), tiles, order;  // rangeSymbols: what the tiles of element i have to cover (0: no tile)
  uint32_t maxBlocks = 0;
  for (uint32_t i = 0; i < B; ++i) {
    // (an element that asks for blocks has tile 0, which reports it, even with no capacity at all)
    const uint32_t blocks = numBlocks[i] ? std::max(1u, std::min(numBlocks[i], divUp(outCapacity[i], kBlockSize))) : 0u;
    rangeSymbols[i] = blocks * kBlockSize;
    maxBlocks = std::max(maxBlocks, blocks);
  }
  LaunchGroup g = decodeRectangle(maxBlocks, false);
  work->assign(firstBlock, firstBlock + B);
  work->insert(work->end(), numBlocks, numBlocks + B);
  g.listed = true;
  g.tilesAt = (uint32_t)work->size();
  if (maxBlocks == 0u) {
    work->push_back(0xffffffffu);  // nothing but empty requests: one workgroup, which reports them
  } else {
    if (!raggedOrder(1, rangeSymbols, g.tileBlocks * kBlockSize, g.maxTiles, 0u, &tiles, &order, work)) return false;
    listTilesTileMajor(order, tiles, g.maxTiles, work);
  }
  g.numTiles = (uint32_t)(work->size() - g.tilesAt);
  *group = g;
  return true;
}

}  // namespace dgpu
