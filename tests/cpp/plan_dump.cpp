// Prints the work plans (csrc/work_plan.h) of a fixed table of batches: every launch group's fields and the whole work
// vector, for encode (raw bytes, bf16, fp32, bf16 cast; with and without a caller's histogram) and decode (whole,
// accumulate, ranged) under every setting of the two test hooks.  tests/test_work_plan.py compares the output with
// tests/plan_dump.expected, which was recorded from the planning code as it stood inside capi.hip.
//   plan_dump          the table
//   plan_dump --time   host time of the planner alone
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../dietgpu_amd/csrc/work_plan.h"

using namespace dgpu;

namespace {

typedef std::vector<uint32_t> Sizes;

Sizes rep(uint32_t n, uint32_t size) { return Sizes(n, size); }
Sizes cat(std::initializer_list<Sizes> parts) {
  Sizes out;
  for (const Sizes& p : parts) out.insert(out.end(), p.begin(), p.end());
  return out;
}
// n sizes of `blocks` blocks each, none of them equal: blocks * 4096 - 7 * i
Sizes blocksOf(uint32_t n, uint32_t blocks) {
  Sizes out(n);
  for (uint32_t i = 0; i < n; ++i) out[i] = blocks * kBlockSize - 7u * i;
  return out;
}

struct Case {
  const char* name;
  Sizes sizes;
};

std::vector<Case> cases() {
  const uint32_t U = 65536;  // two 8-block encoder tiles, one 16-block decoder tile
  std::vector<Case> c;
  c.push_back({"one", {10000}});
  c.push_back({"equal", rep(8, 20000)});
  c.push_back({"single_blocks", {100, 4096, 1, 4000, 2048, 4095, 17, 3000, 4096, 999, 1234, 64}});
  c.push_back({"blocks_1_2_4_9", {4096, 8192, 16384, 36864, 3000, 7000, 15000, 36000}});
  c.push_back({"40_40_40_3_1", cat({blocksOf(40, 1), blocksOf(40, 2), blocksOf(40, 4), blocksOf(3, 9), blocksOf(1, 40)})});
  c.push_back({"300_small_1_large", cat({blocksOf(300, 1), {64u * 8u * kBlockSize}})});
  c.push_back({"smallest_class_31", cat({blocksOf(31, 1), blocksOf(260, 2), blocksOf(2, 9)})});
  c.push_back({"smallest_class_32", cat({blocksOf(32, 1), blocksOf(260, 2), blocksOf(2, 9)})});
  c.push_back({"small_255", cat({{9u * kBlockSize}, blocksOf(255, 1)})});
  c.push_back({"small_256", cat({{9u * kBlockSize}, blocksOf(256, 1)})});
  c.push_back({"rectangle_four_fifths", {4 * U, 4 * U, 4 * U, 2 * U, 2 * U}});
  c.push_back({"rectangle_one_tile_less", {4 * U, 4 * U, 4 * U, 2 * U, 1 * U}});
  c.push_back({"rectangle_one_tile_more", {4 * U, 4 * U, 4 * U, 3 * U, 2 * U}});
  c.push_back({"empty_elements", {0, 5000, 0, 20000, 0, 40000}});
  c.push_back({"all_empty", {0, 0, 0}});
  c.push_back({"equal_tiles_other_sizes", {40000, 60000, 50000, 65536, 33000, 300000, 120000, 70000, 131072, 66000}});
  c.push_back({"batch_65535", rep(65535, 5000)});
  c.push_back({"batch_65536", rep(65536, 5000)});
  c.push_back({"ragged_65535", cat({rep(65534, 5000), {40000}})});
  c.push_back({"class_element_of_65537_tiles", cat({{65537u * 8u * kBlockSize}, blocksOf(300, 1)})});
  c.push_back({"class_element_of_65536_tiles", cat({{65536u * 8u * kBlockSize}, blocksOf(300, 1)})});
  return c;
}

// (an unlisted group -- a rectangle -- has nothing but zeros in its list fields: they are checked, not printed)
std::string groupLine(const LaunchGroup& g) {
  char buf[256];
  int n = snprintf(buf, sizeof(buf), "  group tileBlocks=%u max=%u maxTiles=%u", g.tileBlocks, g.maxSize, g.maxTiles);
  const bool zeros = !(g.tilesAt | g.numTiles | g.histAt | g.numHistParts | g.histPartBytes | g.tileBaseAt | g.elemsAt | g.numElems);
  if (!g.listed && zeros) {
    snprintf(buf + n, sizeof(buf) - n, " rectangle\n");
  } else {
    snprintf(buf + n, sizeof(buf) - n, " listed=%d tiles=%u+%u hist=%u+%u/%u tileBase=%u elems=%u+%u\n", (int)g.listed, g.tilesAt, g.numTiles, g.histAt,
             g.numHistParts, g.histPartBytes, g.tileBaseAt, g.elemsAt, g.numElems);
  }
  return buf;
}

// The whole vector, losslessly: a word in hex, or a run of three or more words in arithmetic progression as
// first+step*count (the lists are runs by construction: the tiles of an element step by 1, elements by 0x10000).
std::string workText(const std::vector<uint32_t>& work) {
  std::string out;
  char buf[64];
  snprintf(buf, sizeof(buf), "  work %zu:", work.size());
  out += buf;
  size_t tokens = 0;
  for (size_t i = 0; i < work.size();) {
    size_t n = 1;
    const uint32_t step = i + 1 < work.size() ? work[i + 1] - work[i] : 0u;
    while (i + n < work.size() && work[i + n] - work[i + n - 1] == step) ++n;
    if (n >= 3) {
      snprintf(buf, sizeof(buf), "%x+%x*%zu", work[i], step, n);
    } else {
      n = 1;
      snprintf(buf, sizeof(buf), "%x", work[i]);
    }
    out += (tokens && tokens % 12 == 0 ? "\n   " : " ") + std::string(buf);
    ++tokens;
    i += n;
  }
  return out + "\n";
}

std::string planText(const std::vector<LaunchGroup>& groups, const std::vector<uint32_t>& work) {
  std::string out;
  for (const LaunchGroup& g : groups) out += groupLine(g);
  return out + workText(work);
}

// The calls of one batch that share a plan are named together in front of it, each call with the settings of the two
// hooks (work lists, size classes; '-' = -1) under which it gets that plan: "decode[-- -0 -1]".
struct CasePlans {
  std::vector<std::string> plans;                                          // in order of first appearance
  std::vector<std::vector<std::pair<std::string, std::string>>> members;  // per plan: (call, settings) in order
  void add(const std::string& call, const std::string& setting, const std::string& plan) {
    size_t k = 0;
    while (k < plans.size() && plans[k] != plan) ++k;
    if (k == plans.size()) plans.push_back(plan), members.emplace_back();
    if (members[k].empty() || members[k].back().first != call) members[k].push_back({call, setting});
    else members[k].back().second += " " + setting;
  }
  void print(const char* name) const {
    for (size_t k = 0; k < plans.size(); ++k) {
      std::string line = std::string(name) + ":";
      for (const auto& m : members[k]) {
        const std::string item = " " + m.first + "[" + m.second + "]";
        if (line.size() + item.size() > 140) printf("%s\n", line.c_str()), line = " ";
        line += item;
      }
      printf("%s\n%s", line.c_str(), plans[k].c_str());
    }
  }
};

void dumpTable() {
  struct Enc {
    const char* name;
    uint32_t ft;
  };
  const Enc encs[] = {{"raw", 0u}, {"bf16", kBFloat16}, {"fp32", kFloat32}, {"bf16cast", kBFloat16 | kCastSource}};
  const char mode[] = "-01";
  for (const Case& c : cases()) {
    uint32_t maxSize = 0;
    for (uint32_t s : c.sizes) maxSize = std::max(maxSize, s);
    CasePlans plans;
    std::vector<LaunchGroup> groups;
    auto each = [&](const std::string& call, auto plan) {
      for (int lists = -1; lists <= 1; ++lists) {
        for (int classes = -1; classes <= 1; ++classes) {
          PlanPolicy policy;
          policy.workLists = lists, policy.sizeClasses = classes;
          std::vector<uint32_t> work;
          plan(policy, &work);
          plans.add(call, std::string{mode[lists + 1], mode[classes + 1]}, planText(groups, work));
        }
      }
    };
    for (const Enc& e : encs) {
      for (int hist = 0; hist < 2; ++hist) {
        each(std::string(e.name) + (hist ? "+hist" : ""), [&](const PlanPolicy& policy, std::vector<uint32_t>* work) {
          planEncodeCall(policy, c.sizes, e.ft, maxSize, hist != 0, &groups, work);
        });
      }
    }
    for (int whole = 1; whole >= 0; --whole) {
      each(whole ? "decode" : "accumulate", [&](const PlanPolicy& policy, std::vector<uint32_t>* work) {
        planDecodeCall(policy, c.sizes, maxSize, whole != 0, &groups, work);
      });
    }
    plans.print(c.name);
  }
  // ranged decode: {firstBlock, numBlocks, outCapacity} per element
  struct Range {
    const char* name;
    std::vector<uint32_t> first, num, cap;
  };
  const uint32_t K = kBlockSize;
  const Range ranges[] = {
      {"mixed_4_block_tiles", {0, 3, 100, 7, 0}, {1, 8, 2, 0, 5}, {K, 8 * K, 2 * K, 9 * K, 3 * K + 1}},
      {"mixed_16_block_tiles", {0, 3, 100, 7, 0, 2}, {1, 40, 2, 0, 9, 17}, {K, 40 * K, 2 * K, 9 * K, 9 * K, 16 * K}},
      {"all_empty", {0, 5, 9}, {0, 0, 0}, {K, 0, 100 * K}},
      {"to_the_end", {0, 4, 1}, {0xffffffffu, 0xffffffffu, 0xffffffffu}, {5 * K, 20 * K + 5, 0}},
      {"one", {2}, {3}, {3 * K}},
      {"capacity_limit", {0, 0}, {0xffffffffu, 1}, {0xfffff000u, K}},
  };
  for (const Range& r : ranges) {
    std::vector<LaunchGroup> groups(1);
    std::vector<uint32_t> work;
    const bool ok = planRangeCall((uint32_t)r.first.size(), r.first.data(), r.num.data(), r.cap.data(), &groups[0], &work);
    printf("range %s\n%s", r.name, ok ? planText(groups, work).c_str() : "  refused\n");
  }
}

// ns per call of the encode planner (the decode planner shares everything it times)
double timePlan(const std::vector<Sizes>& batches, int reps) {
  PlanPolicy policy;
  std::vector<LaunchGroup> groups;
  size_t sink = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < reps; ++i) {
    const Sizes& s = batches[(size_t)i % batches.size()];
    std::vector<uint32_t> work;
    planEncodeCall(policy, s, kBFloat16, s[0], false, &groups, &work);
    sink += work.size() + groups.size();
  }
  const auto t1 = std::chrono::steady_clock::now();
  if (sink == 1) printf(" ");
  return std::chrono::duration<double, std::nano>(t1 - t0).count() / reps;
}
void timeTable() {
  // 32 769 mixed sizes: one large tensor in front (the largest: timePlan takes sizes[0] for maxSize) and 2 / 1 / 4-block ones
  Sizes mixed{64u * 8u * kBlockSize}, other;
  for (uint32_t i = 0; i < 32768; ++i) mixed.push_back(i % 3 == 0 ? 8000u : (i % 3 == 1 ? 3000u + i % 1000u : 16000u));
  other = mixed;
  other[5] += 1;  // (two batches in turn: every call misses the one-entry cache)
  for (int round = 0; round < 3; ++round) {
    printf("equal_256 %.0f ns  mixed_32769_miss %.0f ns  mixed_32769_hit %.0f ns\n", timePlan({rep(256, 512 * 1024)}, 20000),
           timePlan({mixed, other}, 200), timePlan({mixed}, 2000));
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "--time") == 0) {
    timeTable();
  } else {
    dumpTable();
  }
  return 0;
}
