// rANS decode for gfx950, with the float join fused into the write-out.
//
// Behavioural contract: ansDecodeTable / ansDecodeKernel / decodeOneWarp
// (dietgpu/ans/GpuANSDecode.cuh:34-476) and JoinFloatWriter / FloatOutProvider
// (dietgpu/float/GpuFloatDecompress.cuh:320-521).  Organisation for wave64:
//
//   * one wave64 decodes TWO 4 KiB blocks (lanes 0-31 / 32-63), one 64-bit
//     ballot per row; readers take their words from the top of the block down
//     in descending column order (the mirror of the encoder's ascending
//     emission order);
//   * the row loop is a dependent chain -- LUT entry (LDS), state update,
//     ballot, word address, word (LDS), renormalise -- and costs what that
//     chain's latency costs divided by the wavefronts that fit (DESIGN.md
//     section 3: extra instructions beside the chain are nearly free), so:
//       - the decode LUT holds 64-bit entries {pdf | sym << 24, x - cdf}: the
//         state update is one shift + one v_mad_u32_u24, and the symbol is
//         already in the top byte where the write-out wants it;
//       - compressed words sit in a 2 KiB LDS region per block: the whole
//         block when both blocks of the wave have <= 1024 words, else a ring of
//         4 x 512-byte chunks refilled one 8-row group ahead -- not a
//         worst-case 5 KiB stage, so LDS does not cap occupancy harder;
//       - the unread-word positions of the two halves are wave-uniform and live
//         in SGPRs (s_bcnt1 of the ballot halves); a lane's rank comes from
//         v_mbcnt_lo/hi over the ballot;
//       - aligned 16-bit float outputs: a row leaves {sym, 0} in a 512-byte LDS
//         buffer (ds_write_b16_d16_hi, no VALU); every 8 rows a lane joins its
//         8 consecutive words with the 8 non-compressed bytes it fetched with
//         ONE load and stores 16 bytes (RowSink::flushGroup).  Otherwise the
//         per-row sinks join and store one element per lane and row.
#pragma once
#include <type_traits>

#include "format.h"
#include "plan_constants.h"
#include "kernels_stats.h"

namespace dgpu {

// Locates the ANS archive of batch element b (skipping the float header and
// non-comp plane for float archives, FloatANSProvider,
// GpuFloatDecompress.cuh:320-351).
__device__ __forceinline__ const uint8_t* locateAns(const uint8_t* archive, uint32_t ft, uint32_t* floatSize) {
  if (!ft) return archive;
  const FloatHeader fh = *(const FloatHeader*)archive;
  if (floatSize) *floatSize = fh.size;
  return archive + 16u + floatUncompDataSize(ft, fh.size);
}

// ---------------------------------------------------------------------------
struct DecodeArgs {
  BatchView in;            // archive pointers
  BatchView out;           // output pointers + capacities (bytes for raw, float words for float)
  uint32_t floatType;      // must equal the template FT
  uint8_t* outSuccess;     // [B] nullable
  uint32_t* outSize;       // [B] nullable
  const uint32_t* inBytes; // [B] nullable: bytes available at in.ptr(b) (the *_bounded entry points); an archive
                           // that claims to be longer is rejected instead of being read past its buffer
  uint32_t numInBatch;     // B
  uint32_t maxTiles;       // k_ans_decode: tiles per element the 1-D grid is laid out for
  uint32_t order;          // k_ans_decode: how workgroup index -> (element, tile), see decodeTileOf
  uint32_t uniformInBytes; // != 0 (and inBytes == nullptr): every archive has this many bytes available (stride batches)
  const uint32_t* workMap; // kDecOrderMap: [grid] element << 16 | tile, the tiles that exist (the host knows the capacities);
                           // k_ans_decode_pair: [numListed] the elements to pair up
  uint32_t numListed;      // k_ans_decode_pair with a workMap: its entries
  // k_ans_decode_range only (see decodeTile): blocks [firstBlock[b], firstBlock[b] + numBlocks[b]) of element b
  const uint32_t* firstBlock = nullptr;  // [B]
  const uint32_t* numBlocks = nullptr;   // [B]; 0xffffffff = to the end of the element
  // k_ans_decode_accum only: out holds float32 accumulators; 0: acc = decoded (the accumulator is not read), 1: acc += decoded
  uint32_t accumulate = 0;
  // k_ans_decode_reduce only: in / inBytes hold numInBatch * numSources entries, source s of member b at b * numSources + s
  uint32_t numSources = 1;
  // k_ans_decode_reduce_stats only: [numInBatch][256] counts of the exponent bytes of the stored sums, rounded to the
  // archive type (zero at launch; see decodeReduceTile, kStats)
  uint32_t* stats = nullptr;
  // the scaled forms of k_ans_decode_reduce_mixed / _mixed_stats only: acc = fl32(sum * scale) on the last source's store
  // (finite, not zero, not 1: the host launches the unscaled kernels for 1; see decodeReduceTile, kScaled)
  float scale = 1.0f;
  // the norm forms (k_ans_decode_reduce_mixed_norm / _mixed_stats_norm) only: one partial per (member, tile), slot
  // b * maxTiles + tile, zero at launch -- the squared norm of the tile's finite measured words and, behind the
  // numInBatch * maxTiles float64, the counts of its non-finite ones (decodeReduceTile, kNorm); k_reduce_norm_finish
  // adds a member's partials in tile order
  double* normPartials = nullptr;
  // k_ans_decode_scaled and k_ans_decode_accum_scaled: the factor of member b is scalePtr[b * scaleStride] (device
  // memory, read when the kernel runs; scaleStride 0: one factor for the call, 1: one per member), or `scale` above when
  // scalePtr is null
  const float* scalePtr = nullptr;
  uint32_t scaleStride = 0;
  // k_ans_decode_update only: the seed of the stochastic rounding is *seedPtr (device memory, 8-byte aligned, read when
  // the kernel runs) or `seed` when seedPtr is null; member b draws the random bits of member firstMember + b
  uint32_t firstMember = 0;
  uint64_t seed = 0;
  const uint64_t* seedPtr = nullptr;
};
__device__ __forceinline__ uint64_t decodeInBytes(const DecodeArgs& a, uint32_t b) {
  return a.inBytes ? (uint64_t)a.inBytes[b] : (a.uniformInBytes ? (uint64_t)a.uniformInBytes : ~0ull);
}

// Workgroup index -> (element, tile) of k_ans_decode's 1-D grid of B * maxTiles workgroups (kDecOrderXcd: B rounded up to 8).  The hardware
// dispatches workgroups in index order, workgroup w on XCD w mod 8 (docs/HISTORY.md section 3).
//   kDecOrderElementMajor: w = b * T + tile -- the tiles of an element run back to back (rounds 1-4)
//   kDecOrderTileMajor:    w = tile * B + b -- the order the encoder wrote the archives in
//   kDecOrderXcd:          every XCD walks ITS elements (b mod 8 == XCD) element-major: consecutive workgroups touch
//                          eight elements, and an element's header, pdf table and descriptors stay in one XCD's L2
//   kDecOrderMap:          batches whose capacities differ widely: the grid holds only the tiles inside each element's
//                          capacity, listed by the host (a rectangle laid out for the largest element would be mostly
//                          workgroups that start, find nothing and leave)
constexpr uint32_t kDecOrderElementMajor = 0, kDecOrderTileMajor = 1, kDecOrderXcd = 2, kDecOrderMap = 3;
__device__ __forceinline__ bool decodeTileOf(const DecodeArgs& a, uint32_t w, uint32_t* b, uint32_t* tile) {
  const uint32_t T = a.maxTiles, B = a.numInBatch;
  if (a.order == kDecOrderMap) {
    const uint32_t m = a.workMap[w];
    *b = m >> 16;
    *tile = m & 0xffffu;
    return true;
  }
  if (a.order == kDecOrderTileMajor) {
    *tile = w / B;
    *b = w - *tile * B;
    return *tile < T;
  }
  if (a.order == kDecOrderXcd) {
    const uint32_t x = w & 7u, g = w >> 3;
    const uint32_t e = g / T;
    *tile = g - e * T;
    *b = e * 8u + x;
    return *b < B;
  }
  *b = w / T;
  *tile = w - *b * T;
  return *b < B;
}

// ---------------------------------------------------------------------------
// Per-row sinks.  Each lane owns element row * 32 + hl of its block.  `e0` is
// LUT word 0 = pdf | sym << 24.  The float joins are FloatTypeInfo<FT>::join
// (GpuFloatUtils.cuh:117-119,149-159,187-190) arranged so that the result sits
// in the TOP half of a register and is stored with a d16_hi short store; the
// pdf bits that ride along in the low 12 bits never reach the stored half.
// Wide stores: with one 2-byte (1-byte) store per lane and row a half-wave writes 64-byte (32-byte) pieces, which
// the memory system turns into 1.3x the bytes (WRITE_SIZE, profiles/r02_write_calib.txt).  Instead the 8 rows of a
// group are transposed through a 512-byte LDS buffer per block and leave as ONE 16-byte (8-byte) store per lane:
// 512 (256) contiguous bytes (bf16 P=10 decode 100 -> 86 us, WRITE_SIZE back to the algorithmic bytes).  fp32 rows
// are 128-byte pieces already; raw bytes in 16-block tiles keep the narrow stores (decXposeBytes).
__device__ __forceinline__ uint2 decLoad8(const uint8_t* p) {
  typedef uint32_t u32x2n __attribute__((ext_vector_type(2)));
  if (kNtDecLoads) {
    const u32x2n v = __builtin_nontemporal_load((const u32x2n*)p);
    return make_uint2(v.x, v.y);
  }
  return *(const uint2*)p;
}
__host__ __device__ constexpr uint32_t decOutWordBytes(uint32_t ft) { return ft == 0u ? 1u : (ft == kFloat32 ? 4u : 2u); }
__device__ __forceinline__ uint4 decLoad16(const uint8_t* p) { return streamLoad<kNtDecLoads>((const uint4*)p); }
typedef __attribute__((address_space(3))) uint16_t LdsU16w;
typedef uint32_t u32x4w __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4w LdsU4w;

// Per-row join (narrow path): {e0.b3 (symbol), r.b0 (non-compressed byte), e0.b1, e0.b0} in one v_perm_b32.
// (The byte loaded a group earlier still costs one v_and per row here: it crosses the loop edge as an i8 and the
// compiler sinks its zero-extension away from the load.  The wide path has no per-row byte at all.)
__device__ __forceinline__ uint32_t joinBytes(uint32_t e0, uint32_t r) { return __builtin_amdgcn_perm(e0, r, 0x07000504u); }

template <uint32_t FT>
struct RowSink;

template <>
struct RowSink<0> {  // raw bytes (BatchWriter, BatchProvider.cuh:16-37)
  uint8_t* out;
  __device__ __forceinline__ void init(uint8_t* outBase, const uint8_t*, uint32_t, size_t first, uint32_t hl) {
    out = outBase + first + hl;
  }
  typedef uint32_t Pre;
  typedef uint2 GroupPre;
  __device__ __forceinline__ uint32_t prefetch(uint32_t) const { return 0; }
  __device__ __forceinline__ void store(uint32_t row, uint32_t e0, uint32_t) const {
    out[row * 32u] = (uint8_t)(e0 >> 24);  // 32-byte row pieces: left to the L2 to merge
  }
  // wide-store variant: every row leaves the TOP half of LUT word 0 ({sym, 0}) in a 512-byte LDS buffer as it is
  // (ds_write_b16_d16_hi: no VALU in the row); a lane then holds 8 consecutive symbols as four {sym, 0, sym, 0}
  // dwords, packs them with two v_perm_b32 and stores 8 bytes
  static constexpr uint32_t kXposeBytes = 512;
  __device__ __forceinline__ uint2 prefetchGroup(uint32_t, uint32_t) const { return make_uint2(0, 0); }
  __device__ __forceinline__ void stageRow(uint32_t xpose, uint32_t j, uint32_t hl, uint32_t e0) const {
    *(LdsU16w*)(uintptr_t)(xpose + (j * 32u + hl) * 2u) = (uint16_t)(e0 >> 16);
  }
  __device__ __forceinline__ void flushGroup(uint32_t xpose, uint32_t g, uint32_t hl, uint2) const {
    typedef uint32_t u32x2l __attribute__((ext_vector_type(2)));
    const u32x4w v = *(const LdsU4w*)(uintptr_t)(xpose + hl * 16u);
    const uint32_t o0 = __builtin_amdgcn_perm(v.y, v.x, 0x07050301u);  // {x.b1, x.b3, y.b1, y.b3}
    const uint32_t o1 = __builtin_amdgcn_perm(v.w, v.z, 0x07050301u);
    *(u32x2l*)(out - hl + g * 256u + hl * 8u) = u32x2l{o0, o1};
  }
};

template <>
struct RowSink<kFloat16> {  // word = comp << 8 | nonComp
  uint16_t* out;
  const uint8_t* nc;
  __device__ __forceinline__ void init(uint8_t* outBase, const uint8_t* archive, uint32_t, size_t first, uint32_t hl) {
    out = (uint16_t*)outBase + first + hl;
    nc = archive + 16u + first + hl;
  }
  typedef uint32_t Pre;
  typedef uint2 GroupPre;
  __device__ __forceinline__ uint32_t prefetch(uint32_t row) const { return nc[row * 32u]; }
  // the joined word in the TOP half
  static __device__ __forceinline__ uint32_t joinWord(uint32_t e0, uint32_t r) { return joinBytes(e0, r); }  // [sym][nc][0000 pdf]
  __device__ __forceinline__ void store(uint32_t row, uint32_t e0, uint32_t r) const {
    const uint32_t v = joinWord(e0, r);
    streamStore<kNtDecStores>(&out[row * 32u], (uint16_t)(v >> 16));
  }
  // wide variant (see decodeBlock): rows stage {sym, 0}; a lane joins its 8 consecutive words with the 8
  // non-compressed bytes it loaded with ONE 8-byte load: one v_perm_b32 per pair of words
  static constexpr uint32_t kXposeBytes = 512;
  __device__ __forceinline__ uint2 prefetchGroup(uint32_t g, uint32_t hl) const { return decLoad8(nc - hl + g * 256u + hl * 8u); }
  __device__ __forceinline__ void stageRow(uint32_t xpose, uint32_t j, uint32_t hl, uint32_t e0) const {
    *(LdsU16w*)(uintptr_t)(xpose + (j * 32u + hl) * 2u) = (uint16_t)(e0 >> 16);
  }
  // the lane's 8 consecutive words of the group, two per dword
  static __device__ __forceinline__ u32x4w joinGroup(uint32_t xpose, uint32_t hl, uint2 ncb) {
    const u32x4w v = *(const LdsU4w*)(uintptr_t)(xpose + hl * 16u);
    u32x4w o;
    o.x = __builtin_amdgcn_perm(v.x, ncb.x, 0x07010500u);  // {nc0, sym0, nc1, sym1}
    o.y = __builtin_amdgcn_perm(v.y, ncb.x, 0x07030502u);
    o.z = __builtin_amdgcn_perm(v.z, ncb.y, 0x07010500u);
    o.w = __builtin_amdgcn_perm(v.w, ncb.y, 0x07030502u);
    return o;
  }
  __device__ __forceinline__ void flushGroup(uint32_t xpose, uint32_t g, uint32_t hl, uint2 ncb) const {
    const u32x4w o = joinGroup(xpose, hl, ncb);
    u32x4w* dst = (u32x4w*)(out - hl + g * 256u + hl * 8u);
    if (kNtDecStores) __builtin_nontemporal_store(o, dst);
    else *dst = o;
  }
};

template <>
struct RowSink<kBFloat16> {  // word = (comp << 8 | nonComp) >> 1 | (nonComp & 1) << 15
  uint16_t* out;
  const uint8_t* nc;
  __device__ __forceinline__ void init(uint8_t* outBase, const uint8_t* archive, uint32_t, size_t first, uint32_t hl) {
    out = (uint16_t*)outBase + first + hl;
    nc = archive + 16u + first + hl;
  }
  typedef uint32_t Pre;
  typedef uint2 GroupPre;
  __device__ __forceinline__ uint32_t prefetch(uint32_t row) const { return nc[row * 32u]; }
  // the joined word in the TOP half
  static __device__ __forceinline__ uint32_t joinWord(uint32_t e0, uint32_t r) {
    const uint32_t lo = joinBytes(e0, r);                                 // [sym][nc][0000 pdf]
    return __builtin_amdgcn_alignbit(r, lo, 1);                 // (lo >> 1) | (r << 31)
  }
  __device__ __forceinline__ void store(uint32_t row, uint32_t e0, uint32_t r) const {
    const uint32_t v = joinWord(e0, r);
    streamStore<kNtDecStores>(&out[row * 32u], (uint16_t)(v >> 16));                    // [sign][exp][mant7]
  }
  // wide variant: as fp16, then every 16-bit half {exp, nc} rotated right by one (sign to the top):
  // (h >> 1) + h * 2^15 on packed halves (v_pk_lshrrev_b16 + v_pk_mad_u16)
  static constexpr uint32_t kXposeBytes = 512;
  __device__ __forceinline__ uint2 prefetchGroup(uint32_t g, uint32_t hl) const { return decLoad8(nc - hl + g * 256u + hl * 8u); }
  __device__ __forceinline__ void stageRow(uint32_t xpose, uint32_t j, uint32_t hl, uint32_t e0) const {
    *(LdsU16w*)(uintptr_t)(xpose + (j * 32u + hl) * 2u) = (uint16_t)(e0 >> 16);
  }
  static __device__ __forceinline__ uint32_t rotrHalves(uint32_t x) {
    typedef uint16_t u16x2w __attribute__((ext_vector_type(2)));
    const u16x2w h = __builtin_bit_cast(u16x2w, x);
    const uint32_t shifted = __builtin_bit_cast(uint32_t, (u16x2w)(h >> 1));
    uint32_t r;
    asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(r) : "v"(x), "s"(0x80008000u), "v"(shifted));
    return r;
  }
  // the lane's 8 consecutive words of the group, two per dword
  static __device__ __forceinline__ u32x4w joinGroup(uint32_t xpose, uint32_t hl, uint2 ncb) {
    const u32x4w v = *(const LdsU4w*)(uintptr_t)(xpose + hl * 16u);
    u32x4w o;
    o.x = rotrHalves(__builtin_amdgcn_perm(v.x, ncb.x, 0x07010500u));
    o.y = rotrHalves(__builtin_amdgcn_perm(v.y, ncb.x, 0x07030502u));
    o.z = rotrHalves(__builtin_amdgcn_perm(v.z, ncb.y, 0x07010500u));
    o.w = rotrHalves(__builtin_amdgcn_perm(v.w, ncb.y, 0x07030502u));
    return o;
  }
  __device__ __forceinline__ void flushGroup(uint32_t xpose, uint32_t g, uint32_t hl, uint2 ncb) const {
    const u32x4w o = joinGroup(xpose, hl, ncb);
    u32x4w* dst = (u32x4w*)(out - hl + g * 256u + hl * 8u);
    if (kNtDecStores) __builtin_nontemporal_store(o, dst);
    else *dst = o;
  }
};

template <>
struct RowSink<kFloat32> {  // rotr32(comp << 24 | nonComp24, 1)
  uint32_t* out;
  const uint16_t* nc2;  // u16 plane of roundUp(size, 8) entries
  const uint8_t* nc1;   // then the high-byte plane
  __device__ __forceinline__ void init(uint8_t* outBase, const uint8_t* archive, uint32_t floatSize, size_t first, uint32_t hl) {
    out = (uint32_t*)outBase + first + hl;
    nc2 = (const uint16_t*)(archive + 16u) + first + hl;
    nc1 = archive + 16u + 2u * (size_t)roundUp(floatSize, 8u) + first + hl;
  }
  typedef uint32_t Pre;
  typedef uint2 GroupPre;
  __device__ __forceinline__ uint32_t prefetch(uint32_t row) const {
    return ((uint32_t)nc1[row * 32u] << 16) | nc2[row * 32u];
  }
  __device__ __forceinline__ void store(uint32_t row, uint32_t e0, uint32_t r) const {
    const uint32_t v = (e0 & 0xff000000u) | r;
    streamStore<kNtDecStores>(&out[row * 32u], (uint32_t)__builtin_amdgcn_alignbit(v, v, 1));
  }
  // the same word for AccumSink (store() keeps its own text: routing it through here reorders its row loop's schedule)
  static __device__ __forceinline__ uint32_t joinWord(uint32_t e0, uint32_t r) {
    const uint32_t v = (e0 & 0xff000000u) | r;
    return (uint32_t)__builtin_amdgcn_alignbit(v, v, 1);
  }
  static constexpr uint32_t kXposeBytes = 0;  // 128-byte row pieces already: no transposition
  __device__ __forceinline__ uint2 prefetchGroup(uint32_t, uint32_t) const { return make_uint2(0, 0); }
  __device__ __forceinline__ void stageRow(uint32_t, uint32_t, uint32_t, uint32_t) const {}
  __device__ __forceinline__ void flushGroup(uint32_t, uint32_t, uint32_t, uint2) const {}
};

// ---------------------------------------------------------------------------
// Accumulating sinks (k_ans_decode_accum): the interface of RowSink<FT>, but the joined word is widened to float32 and
// goes to a float32 accumulator: acc = widened (accumulate == 0: the accumulator is not read) or acc += widened -- one
// IEEE float32 add, round to nearest even, denormals kept, nothing to contract it with.  Widening is exact: fp16 ->
// v_cvt_f32_f16 (fp16 denormals become float32 normals), bf16 -> word << 16, fp32 as it is.  `accumulate` is uniform
// over the launch.  The accumulator words a lane adds to are requested where RowSink requests the non-compressed bytes
// of the same rows -- two 8-row groups ahead on the wide path, one otherwise -- and travel with them (GroupPre / Pre),
// so the row loop does not wait for them.  Wide path (16-bit types): a lane's 8 consecutive words leave as 32
// contiguous bytes (two 16-byte stores) where RowSink leaves 16.
template <uint32_t FT>
__device__ __forceinline__ float accWiden16(uint32_t h);  // h: the 16-bit word in the LOW half
template <>
__device__ __forceinline__ float accWiden16<kFloat16>(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }
template <>
__device__ __forceinline__ float accWiden16<kBFloat16>(uint32_t h) { return __builtin_bit_cast(float, h << 16); }
// (__fadd_rn: never fused, whatever the contraction mode of the translation unit)
__device__ __forceinline__ uint32_t accAdd(uint32_t acc, float v) { return __builtin_bit_cast(uint32_t, __fadd_rn(__builtin_bit_cast(float, acc), v)); }
typedef u32x4w u32x4w4 __attribute__((aligned(4)));  // accumulators are float-aligned only

struct AccumPre {  // one row: the non-compressed byte(s) and the accumulator word
  uint32_t r, acc;
  __device__ __forceinline__ AccumPre() = default;
  __device__ __forceinline__ AccumPre(uint32_t) : r(0), acc(0) {}
};
struct AccumGroupPre {  // one 8-row group of a lane: 8 non-compressed bytes and 8 accumulator words
  uint2 nc;
  u32x4w a0, a1;
};

// kSlots != 0 (k_ans_decode_reduce_stats): every float32 word the sink stores is also rounded to FT (castRound, the cast
// encoder's own rounding) and the exponent byte of the rounded word -- the encoder's split: fp16 w >> 8, bf16 bits
// 14..7 -- is counted in the workgroup's LDS bins, in this lane's slot column `bins` (an LDS address; bin c at
// bins + c * kSlots * 4; 0: this is not the last source, nothing is counted).  Counting sits inside store() and
// flushGroup(), which run for the lanes that store and for no others: the counts of a member add up to its words.
constexpr uint32_t kStatsSlotsLarge = 16, kStatsSlotsSmall = 8;  // lane slots per bin: 16-block / 4-block tiles
__host__ __device__ constexpr uint32_t decStatsSlots(uint32_t tileBlocks) { return tileBlocks <= 4u ? kStatsSlotsSmall : kStatsSlotsLarge; }
__host__ __device__ constexpr uint32_t decStatsBinBytes(uint32_t tileBlocks) { return kNumSymbols * decStatsSlots(tileBlocks) * 4u; }
typedef __attribute__((address_space(3))) uint32_t LdsU32w;
template <bool kStats>
struct AccumBins {};
template <>
struct AccumBins<true> {
  uint32_t bins;
};

// kScaled (the scaled forms of the mixed reduce kernels): on the LAST source the word about to be stored is multiplied by
// the call's scale -- one IEEE float32 multiply after the add, before the store and before count(), so the value counted
// is the value stored.  Where the factor lives: the plain sinks have registers to spare and keep it beside a flag for
// the last source (AccumScale<true>); the counting sink has none (128 VGPRs, the scalar file full: a member, or a
// reload from the kernel arguments, spills a scalar into a VGPR lane, 129) and reads it from LDS, one float per slot
// column directly behind the bins, through the address it already holds: at bins + kNumSymbols * kSlots * 4.  Its
// `bins` is non-zero on the last source and on no other, which is the flag.
template <bool kInRegisters>
struct AccumScale {};
template <>
struct AccumScale<true> {
  float scale;
  uint32_t scaleLast;  // wave-uniform: this is the last source
};
typedef __attribute__((address_space(3))) float LdsF32w;
// (__fmul_rn: never contracted)
__device__ __forceinline__ uint32_t accScale(uint32_t o, float f) { return __builtin_bit_cast(uint32_t, __fmul_rn(__builtin_bit_cast(float, o), f)); }

// kPreScaled (k_ans_decode_accum_scaled): the WIDENED word is multiplied by the member's factor before the add --
// acc = [acc +] fl32(widened * factor): one IEEE float32 multiply and one IEEE add, each rounded once, never an FMA.
// The factor is wave-uniform, set by decodeTile, and lives in a register: the plain sinks only (see above).  The pair is
// written with contraction switched off: __fmul_rn and __fadd_rn are the plain operators in the HIP headers, and a
// multiply that feeds an add is otherwise fused into one FMA by the translation unit's contraction mode.
__device__ __forceinline__ float accMulUnfused(float v, float f) {
#pragma clang fp contract(off)
  return v * f;
}
__device__ __forceinline__ uint32_t accAddUnfused(uint32_t acc, float p) {
#pragma clang fp contract(off)
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, acc) + p);
}
template <bool kHasFactor>
struct AccumFactor {};
template <>
struct AccumFactor<true> {
  float preFactor;
};

// kUnitAware (the norm forms, which serve a factor of 1 as well): the counting sink multiplies by a factor other than 1
// only, so that a factor of 1 leaves the bits of the unscaled call (a multiply by 1 quiets a signalling NaN).  The
// plain sinks need nothing: their flag is simply not set (reduceScales).
template <uint32_t FT, uint32_t kSlots = 0, bool kScaledSink = false, bool kUnitAware = false, bool kPreScaled = false>
struct AccumSink : AccumBins<kSlots != 0u>, AccumScale<kScaledSink && kSlots == 0u>, AccumFactor<kPreScaled> {  // kFloat16 / kBFloat16
  static_assert(FT == kFloat16 || FT == kBFloat16, "");
  static_assert(!kPreScaled || (kSlots == 0u && !kScaledSink), "the pre-scaled sink is a plain sink");
  static constexpr bool kStats = kSlots != 0u;
  static constexpr bool kScaled = kScaledSink;
  static constexpr bool kUnit = kUnitAware;
  static_assert(!kUnitAware || kScaledSink, "");
  static constexpr uint32_t kStatSlots = kSlots;
  __device__ __forceinline__ bool scales() const {
    if constexpr (kStats) return this->bins != 0u;
    else return this->scaleLast != 0u;
  }
  __device__ __forceinline__ float factor() const {
    if constexpr (kStats) return *(LdsF32w*)(uintptr_t)(this->bins + kNumSymbols * kSlots * 4u);
    else return this->scale;
  }
  float* out;
  const uint8_t* nc;
  uint32_t accumulate;
  // kStats: the stored float32 bits `o` enter the histogram of the archive the cast encoder will make of them
  __device__ __forceinline__ void count(uint32_t o) const {
    if constexpr (kStats) {
      const uint32_t c = (castRound<FT>(o) >> (FT == kFloat16 ? 8u : 7u)) & 0xffu;
      __hip_atomic_fetch_add((LdsU32w*)(uintptr_t)(this->bins + c * (kSlots * 4u)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __device__ __forceinline__ void init(uint8_t* outBase, const uint8_t* archive, uint32_t, size_t first, uint32_t hl) {
    out = (float*)outBase + first + hl;
    nc = archive + 16u + first + hl;
  }
  typedef AccumPre Pre;
  typedef AccumGroupPre GroupPre;
  // (prefetchAcc / storeWord, prefetchGroupAcc / flushWords: the halves of prefetch / store and prefetchGroup /
  // flushGroup that do not touch the archive -- a raw source of the mixed reduce hands its words in here)
  __device__ __forceinline__ AccumPre prefetchAcc(uint32_t row) const {
    AccumPre p(0);
    if (accumulate) p.acc = *(const uint32_t*)&out[row * 32u];
    return p;
  }
  // (its own text: forwarding to prefetchAcc puts the accumulator's load in front of the byte's and reschedules the row loops)
  __device__ __forceinline__ AccumPre prefetch(uint32_t row) const {
    AccumPre p(0);
    p.r = nc[row * 32u];
    if (accumulate) p.acc = *(const uint32_t*)&out[row * 32u];
    return p;
  }
  // h: the 16-bit word of FT in the LOW half
  __device__ __forceinline__ void storeWord(uint32_t row, uint32_t h, const AccumPre& p) const {
    float v = accWiden16<FT>(h);
    if constexpr (kPreScaled) v = accMulUnfused(v, this->preFactor);
    uint32_t o;
    if constexpr (kPreScaled) o = accumulate ? accAddUnfused(p.acc, v) : __builtin_bit_cast(uint32_t, v);
    else o = accumulate ? accAdd(p.acc, v) : __builtin_bit_cast(uint32_t, v);
    if constexpr (kScaled && kStats && kUnit) {
      if (scales()) {
        const float f = factor();
        o = f != 1.0f ? accScale(o, f) : o;
      }
    } else if constexpr (kScaled) {
      if (scales()) o = accScale(o, factor());
    }
    streamStore<kNtDecStores>((uint32_t*)&out[row * 32u], o);
    if constexpr (kStats) {
      if (this->bins) count(o);
    }
  }
  __device__ __forceinline__ void store(uint32_t row, uint32_t e0, const AccumPre& p) const {
    storeWord(row, RowSink<FT>::joinWord(e0, p.r) >> 16, p);
  }
  static constexpr uint32_t kXposeBytes = 512;
  __device__ __forceinline__ void prefetchGroupAcc(uint32_t g, uint32_t hl, AccumGroupPre& p) const {
    p.a0 = p.a1 = u32x4w{0u, 0u, 0u, 0u};
    if (accumulate) {
      const u32x4w4* src = (const u32x4w4*)(out - hl + g * 256u + hl * 8u);
      p.a0 = src[0];
      p.a1 = src[1];
    }
  }
  __device__ __forceinline__ AccumGroupPre prefetchGroup(uint32_t g, uint32_t hl) const {
    AccumGroupPre p;
    p.nc = decLoad8(nc - hl + g * 256u + hl * 8u);
    prefetchGroupAcc(g, hl, p);
    return p;
  }
  __device__ __forceinline__ void stageRow(uint32_t xpose, uint32_t j, uint32_t hl, uint32_t e0) const {
    *(LdsU16w*)(uintptr_t)(xpose + (j * 32u + hl) * 2u) = (uint16_t)(e0 >> 16);
  }
  __device__ __forceinline__ void flushGroup(uint32_t xpose, uint32_t g, uint32_t hl, const AccumGroupPre& p) const {
    flushFrom<false>(xpose, g, hl, p, u32x4w{0u, 0u, 0u, 0u});
  }
  // given: the lane's 8 consecutive words of group g, two per dword (joinGroup's layout)
  __device__ __forceinline__ void flushWords(uint32_t g, uint32_t hl, const u32x4w& given, const AccumGroupPre& p) const {
    flushFrom<true>(0u, g, hl, p, given);
  }
  // (one body, the origin of the words a compile-time choice: the decoders' instantiation is flushGroup's text as it was)
  template <bool kGiven>
  __device__ __forceinline__ void flushFrom(uint32_t xpose, uint32_t g, uint32_t hl, const AccumGroupPre& p, const u32x4w& given) const {
    u32x4w w;
    if constexpr (kGiven) w = given;
    else w = RowSink<FT>::joinGroup(xpose, hl, p.nc);
    float v[8];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      v[2u * k] = accWiden16<FT>(w[k] & 0xffffu);
      v[2u * k + 1u] = accWiden16<FT>(w[k] >> 16);
    }
    if constexpr (kPreScaled) {
#pragma unroll
      for (uint32_t k = 0; k < 8u; ++k) v[k] = accMulUnfused(v[k], this->preFactor);
    }
    u32x4w o0, o1;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      if constexpr (kPreScaled) {
        o0[k] = accumulate ? accAddUnfused(p.a0[k], v[k]) : __builtin_bit_cast(uint32_t, v[k]);
        o1[k] = accumulate ? accAddUnfused(p.a1[k], v[4u + k]) : __builtin_bit_cast(uint32_t, v[4u + k]);
      } else {
        o0[k] = accumulate ? accAdd(p.a0[k], v[k]) : __builtin_bit_cast(uint32_t, v[k]);
        o1[k] = accumulate ? accAdd(p.a1[k], v[4u + k]) : __builtin_bit_cast(uint32_t, v[4u + k]);
      }
    }
    if constexpr (kScaled && kStats && kUnit) {
      if (scales()) {
        const float f = factor();
        const bool unit = f == 1.0f;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
          o0[k] = unit ? o0[k] : accScale(o0[k], f);
          o1[k] = unit ? o1[k] : accScale(o1[k], f);
        }
      }
    } else if constexpr (kScaled) {
      if (scales()) {
        const float f = factor();
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
          o0[k] = accScale(o0[k], f);
          o1[k] = accScale(o1[k], f);
        }
      }
    }
    u32x4w4* dst = (u32x4w4*)(out - hl + g * 256u + hl * 8u);
    if (kNtDecStores) {
      __builtin_nontemporal_store(o0, &dst[0]);
      __builtin_nontemporal_store(o1, &dst[1]);
    } else {
      dst[0] = o0;
      dst[1] = o1;
    }
    if constexpr (kStats) {
      if (this->bins) {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
          count(o0[k]);
          count(o1[k]);
        }
      }
    }
  }
};

template <uint32_t kSlots, bool kScaledSink, bool kUnitAware, bool kPreScaled>
struct AccumSink<kFloat32, kSlots, kScaledSink, kUnitAware, kPreScaled> : AccumScale<kScaledSink>, AccumFactor<kPreScaled> {  // row-wise, as RowSink<kFloat32>: 128-byte pieces already
  static_assert(kSlots == 0u, "counting sinks: the 16-bit archive types only");
  static_assert(!kPreScaled || !kScaledSink, "the pre-scaled sink is a plain sink");
  static constexpr bool kStats = false;
  static constexpr bool kScaled = kScaledSink;
  static constexpr bool kUnit = kUnitAware;
  float* out;
  const uint16_t* nc2;
  const uint8_t* nc1;
  uint32_t accumulate;
  __device__ __forceinline__ void init(uint8_t* outBase, const uint8_t* archive, uint32_t floatSize, size_t first, uint32_t hl) {
    out = (float*)outBase + first + hl;
    nc2 = (const uint16_t*)(archive + 16u) + first + hl;
    nc1 = archive + 16u + 2u * (size_t)roundUp(floatSize, 8u) + first + hl;
  }
  typedef AccumPre Pre;
  typedef uint2 GroupPre;
  __device__ __forceinline__ AccumPre prefetch(uint32_t row) const {
    AccumPre p(0);
    p.r = ((uint32_t)nc1[row * 32u] << 16) | nc2[row * 32u];
    if (accumulate) p.acc = *(const uint32_t*)&out[row * 32u];
    return p;
  }
  __device__ __forceinline__ AccumPre prefetchAcc(uint32_t row) const {
    AccumPre p(0);
    if (accumulate) p.acc = *(const uint32_t*)&out[row * 32u];
    return p;
  }
  __device__ __forceinline__ void storeWord(uint32_t row, uint32_t w, const AccumPre& p) const {
    uint32_t o;
    if constexpr (kPreScaled) {
      w = __builtin_bit_cast(uint32_t, accMulUnfused(__builtin_bit_cast(float, w), this->preFactor));
      o = accumulate ? accAddUnfused(p.acc, __builtin_bit_cast(float, w)) : w;
    } else {
      o = accumulate ? accAdd(p.acc, __builtin_bit_cast(float, w)) : w;
    }
    if constexpr (kScaled) {
      if (this->scaleLast != 0u) o = accScale(o, this->scale);
    }
    streamStore<kNtDecStores>((uint32_t*)&out[row * 32u], o);
  }
  __device__ __forceinline__ void store(uint32_t row, uint32_t e0, const AccumPre& p) const {
    storeWord(row, RowSink<kFloat32>::joinWord(e0, p.r), p);
  }
  static constexpr uint32_t kXposeBytes = 0;
  __device__ __forceinline__ uint2 prefetchGroup(uint32_t, uint32_t) const { return make_uint2(0, 0); }
  __device__ __forceinline__ void stageRow(uint32_t, uint32_t, uint32_t, uint32_t) const {}
  __device__ __forceinline__ void flushGroup(uint32_t, uint32_t, uint32_t, uint2) const {}
};

// ---------------------------------------------------------------------------
// Scaling sinks (k_ans_decode_scaled): RowSink<FT> whose joined word is widened to float32 as in the accumulating sinks,
// multiplied by the member's factor -- ONE IEEE float32 multiply (accScale) -- and rounded ONCE back to FT (castRound,
// the cast encoder's rounding: nearest even, float16 denormals produced, overflow to infinity, NaN to a quiet NaN)
// before it is stored where RowSink stores it; float32 rows store the product.  Loads, staging and the shape of the
// stores are RowSink's: the wide path scales the lane's 8 joined words in registers and still leaves ONE 16-byte store.
// The factor is wave-uniform (one per member) and is set by decodeTile, which requests it with the header loads.
template <uint32_t FT>
struct ScaledSink : RowSink<FT> {  // kFloat16 / kBFloat16
  static_assert(FT == kFloat16 || FT == kBFloat16, "");
  float factor;
  // h: the 16-bit word of FT in the LOW half -> the scaled word of FT in the low half
  __device__ __forceinline__ uint32_t scaleWord(uint32_t h) const {
    return castRound<FT>(accScale(__builtin_bit_cast(uint32_t, accWiden16<FT>(h)), factor));
  }
  // two words of FT -> two scaled words of FT
  __device__ __forceinline__ uint32_t scalePair(uint32_t w) const {
    if constexpr (FT == kBFloat16) {
      const uint32_t p0 = accScale(w << 16, factor), p1 = accScale(w & 0xffff0000u, factor);
      return __builtin_amdgcn_perm(castRoundHigh<kBFloat16>(p1), castRoundHigh<kBFloat16>(p0), 0x07060302u);
    } else {
      return __builtin_amdgcn_perm(scaleWord(w >> 16), scaleWord(w & 0xffffu), 0x05040100u);
    }
  }
  __device__ __forceinline__ void store(uint32_t row, uint32_t e0, uint32_t r) const {
    const uint32_t v = RowSink<FT>::joinWord(e0, r);
    streamStore<kNtDecStores>(&this->out[row * 32u], (uint16_t)scaleWord(v >> 16));
  }
  __device__ __forceinline__ void flushGroup(uint32_t xpose, uint32_t g, uint32_t hl, uint2 ncb) const {
    u32x4w o = RowSink<FT>::joinGroup(xpose, hl, ncb);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) o[k] = scalePair(o[k]);
    u32x4w* dst = (u32x4w*)(this->out - hl + g * 256u + hl * 8u);
    if (kNtDecStores) __builtin_nontemporal_store(o, dst);
    else *dst = o;
  }
};
template <>
struct ScaledSink<kFloat32> : RowSink<kFloat32> {
  float factor;
  __device__ __forceinline__ void store(uint32_t row, uint32_t e0, uint32_t r) const {
    streamStore<kNtDecStores>(&this->out[row * 32u], accScale(RowSink<kFloat32>::joinWord(e0, r), factor));
  }
};

// ---------------------------------------------------------------------------
// Updating sinks (k_ans_decode_update; float16 / bfloat16): RowSink<FT> whose joined word is widened to float32,
// multiplied by the member's factor, added to the widened word of the 16-bit TENSOR at the same place (accumulate == 1;
// 0: the tensor is not read) -- ONE IEEE multiply and ONE IEEE add, written unfused as in AccumSink's kPreScaled -- and
// rounded STOCHASTICALLY back to FT (castRoundStochastic) before it is stored where RowSink stores it.  The random bits
// of word k of the member come from srBits(key, k >> 1): `key` is the member's (srMemberKey; wave-uniform, set by
// decodeTile), kLane the index of the lane's word in row 0 of its block.  Staging and the shape of the stores are
// RowSink's: the wide path leaves ONE 16-byte store per lane and group.  The tensor words a lane adds to are requested
// where AccumSink requests its accumulator words -- with the non-compressed bytes, two groups ahead on the wide path --
// as ONE 16-byte load per group (8 words of 2 bytes where AccumSink has 8 of 4), and not at all with accumulate == 0.
typedef u32x4w u32x4w2 __attribute__((aligned(2)));  // tensors are word-aligned only
struct UpdateGroupPre {  // one 8-row group of a lane: 8 non-compressed bytes and 8 tensor words
  uint2 nc;
  u32x4w t;
};
template <uint32_t FT>
struct UpdateSink : RowSink<FT> {
  static_assert(FT == kFloat16 || FT == kBFloat16, "");
  float factor;
  uint32_t accumulate;
  uint32_t key;
  uint32_t kLane;
  __device__ __forceinline__ void init(uint8_t* outBase, const uint8_t* archive, uint32_t floatSize, size_t first, uint32_t hl) {
    RowSink<FT>::init(outBase, archive, floatSize, first, hl);
    kLane = (uint32_t)first + hl;
  }
  typedef AccumPre Pre;
  typedef UpdateGroupPre GroupPre;
  __device__ __forceinline__ AccumPre prefetch(uint32_t row) const {
    AccumPre p(0);
    p.r = this->nc[row * 32u];
    if (accumulate) p.acc = this->out[row * 32u];
    return p;
  }
  // w: the decoded word, t: the tensor word, both float32 bits -> the float32 bits that are rounded
  __device__ __forceinline__ uint32_t value(uint32_t w, uint32_t t) const {
    const float p = accMulUnfused(__builtin_bit_cast(float, w), factor);
    return accumulate ? accAddUnfused(t, p) : __builtin_bit_cast(uint32_t, p);
  }
  __device__ __forceinline__ void store(uint32_t row, uint32_t e0, const AccumPre& p) const {
    const uint32_t h = RowSink<FT>::joinWord(e0, p.r) >> 16;
    const uint32_t v = value(__builtin_bit_cast(uint32_t, accWiden16<FT>(h)), __builtin_bit_cast(uint32_t, accWiden16<FT>(p.acc)));
    const uint32_t k = kLane + row * 32u;
    const uint32_t bits = srBits(key, k >> 1);
    const uint32_t r = (k & 1u) ? bits >> 16 : bits & 0xffffu;
    streamStore<kNtDecStores>(&this->out[row * 32u], (uint16_t)castRoundStochastic<FT>(v, r));
  }
  __device__ __forceinline__ UpdateGroupPre prefetchGroup(uint32_t g, uint32_t hl) const {
    UpdateGroupPre p;
    p.nc = decLoad8(this->nc - hl + g * 256u + hl * 8u);
    p.t = u32x4w{0u, 0u, 0u, 0u};
    if (accumulate) p.t = *(const u32x4w2*)(this->out - hl + g * 256u + hl * 8u);
    return p;
  }
  // two words of FT, the two tensor words under them and the 32 random bits of the pair -> two words of FT
  __device__ __forceinline__ uint32_t updatePair(uint32_t w, uint32_t t, uint32_t bits) const {
    if constexpr (FT == kBFloat16) {
      const uint32_t v0 = value(w << 16, t << 16), v1 = value(w & 0xffff0000u, t & 0xffff0000u);
      return __builtin_amdgcn_perm(castRoundStochasticHigh<kBFloat16>(v1, bits >> 16), castRoundStochasticHigh<kBFloat16>(v0, bits & 0xffffu),
                                   0x07060302u);
    } else {
      const uint32_t v0 = value(__builtin_bit_cast(uint32_t, accWiden16<FT>(w & 0xffffu)), __builtin_bit_cast(uint32_t, accWiden16<FT>(t & 0xffffu)));
      const uint32_t v1 = value(__builtin_bit_cast(uint32_t, accWiden16<FT>(w >> 16)), __builtin_bit_cast(uint32_t, accWiden16<FT>(t >> 16)));
      return __builtin_amdgcn_perm(castRoundStochastic<FT>(v1, bits >> 16), castRoundStochastic<FT>(v0, bits & 0xffffu), 0x05040100u);
    }
  }
  __device__ __forceinline__ void flushGroup(uint32_t xpose, uint32_t g, uint32_t hl, const UpdateGroupPre& p) const {
    u32x4w o = RowSink<FT>::joinGroup(xpose, hl, p.nc);
    const uint32_t pair0 = (kLane - hl + g * 256u + hl * 8u) >> 1;  // the lane's 8 words begin at a multiple of 8
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) o[k] = updatePair(o[k], p.t[k], srBits(key, pair0 + k));
    u32x4w2* dst = (u32x4w2*)(this->out - hl + g * 256u + hl * 8u);
    if (kNtDecStores) __builtin_nontemporal_store(o, dst);
    else *dst = o;
  }
};

// ---------------------------------------------------------------------------
// Compressed-word ring: 4 chunks of 256 words (512 bytes) per block.  Chunk k of
// the block's data lives in slot k & 3.  Words are consumed from the top of the
// block downwards, at most 32 per row = 256 per 8-row group = one chunk per
// group, so at every group boundary the ring (a) receives the chunk requested
// one group earlier and (b) requests the next lower chunk once the unread
// position comes within 512 words of the lowest chunk it holds.  Reads of a
// group stay within 256 words below the position at its start, which the
// protocol guarantees to be resident (proof in DESIGN.md).
typedef __attribute__((address_space(3))) uint16_t LdsU16;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4 LdsU4;
constexpr uint32_t kRingChunkWords = 256;
constexpr uint32_t kRingBytes = 2048;
constexpr uint32_t kGroupRows = 8;

// (blocks per decode workgroup, kDecBlocksPer*Tile: plan_constants.h)
__host__ __device__ constexpr uint32_t decThreads(uint32_t tileBlocks) { return tileBlocks * 32u < 64u ? 64u : tileBlocks * 32u; }
// Store (transposition) buffers per block.  Raw bytes in 16-block tiles keep the narrow stores: a fourth
// workgroup per CU (40 KiB instead of 48: 8 waves per SIMD) is worth more to their row loop than the 8-byte
// stores (256 x 1 MiB Zipf bytes decode 152.5 -> 145 us).  16-bit floats are HBM-bound with the wide stores, and
// their narrow 2-byte non-temporal stores inflate the write traffic by 1.35 (docs/HISTORY.md section 4.2).
__host__ __device__ constexpr uint32_t decXposeBytes(int P, uint32_t ft, uint32_t tileBlocks) {
  (void)P;
  if (ft == 0 && tileBlocks >= 16u) return 0u;
  return ft == kFloat32 ? 0u : 512u;
}
// COMPACT LUT entries, 4 bytes {sym:8 | x - cdf:12 | pdf:12} instead of 8 (two more VALU per row to unpack):
//  * tiles of <= 4 blocks (batches of small elements): residency there is set by the LDS a workgroup needs for
//    its own LUT (measured on 32768 x 4 Ki: decode 228 / 323 / 476 us with a 4 / 8 / 16 KiB LUT; 8192 x 16 Ki:
//    139 -> 133 us), and a lone, latency-bound wavefront does not feel the unpacking;
//  * probBits 11 (any tile): the LUT has 2048 slots; compact, it takes the 8 KiB the 8-byte entries take at
//    probBits 10, which leaves room for the store buffers at the same 3 workgroups per CU (fp16 P=11 decode
//    105.5 -> 97.9 us).  At probBits 10 in 16-block tiles the compact entry is SLOWER (+4 .. +9 us on Zipf bytes):
//    its unpacking sits on the dependent chain.
__host__ __device__ constexpr bool decCompactLut(int P, uint32_t tileBlocks) { return tileBlocks <= 4u || P >= 11; }
__host__ __device__ constexpr uint32_t decLutBytes(int P, uint32_t tileBlocks) {
  return decCompactLut(P, tileBlocks) ? (4u << P) : (8u << P);
}
__host__ __device__ constexpr uint32_t decLdsBytes(int P, uint32_t ft, uint32_t tileBlocks) {
  return decLutBytes(P, tileBlocks) + tileBlocks * kRingBytes + tileBlocks * decXposeBytes(P, ft, tileBlocks);
}

// kIdleUpper (full path only): the upper half of the wave has no block (the element's block count is odd, or
// it has a single block): its lanes run the same straight-line code on don't-care data and only their
// stores are suppressed, so the lower half keeps the fast path instead of the predicated one.
//
// Position tracking (kFull): the unread-word counts of the two halves are wave-uniform, so
// they live in two SGPRs (s_bcnt1 of the ballot halves); a reading lane's word index comes from
// v_mbcnt_lo + v_mbcnt_hi over the 64-bit ballot (lower half: its rank; upper half: rank + readers of the lower
// half) plus one v_mad_i32_i24 that moves the upper half onto its own position: 4-5 VALU per row where the
// per-lane bookkeeping (half select by a 64-bit shift, two popcounts, subtract, mask, shift-add) took 7.
//
// kNoRing (kFull): both blocks of the wave have <= 1024 compressed words (every exponent block of N(0,1)
// bf16 has ~650), so the whole block is staged once and the ring maintenance, the wrap mask and the base OR
// disappear from the row loop (the base is folded into the scalar positions).
// Loads a workgroup issues BEFORE it builds its LUT, so that their round trip to memory overlaps with the build instead
// of following it (k_ans_decode: header -> {pdf, block descriptor, lane states} -> {compressed words, first
// non-compressed bytes} was a chain of four dependent round trips at the start of every workgroup; on cold buffers
// that is 10-15 % of a workgroup's life).  Held in registers across the build; valid for whole-block staging only.
template <typename GroupPre>
struct DecodePreOf {
  uint4 words[4];   // the block's compressed words, 16 bytes per lane and k (kNoRing)
  GroupPre nc[2];   // non-compressed bytes of the last two groups (join at the flush); AccumSink: with their accumulator words
};
typedef DecodePreOf<uint2> DecodePre;
template <uint32_t FT, typename Sink>
__device__ __forceinline__ void decodePrefetch(DecodePreOf<typename Sink::GroupPre>& pre, const uint8_t* __restrict__ gwords, uint32_t numWords,
                                               const Sink& sink, uint32_t hl, bool wide) {
  const uint32_t paddedBytes = roundUp(numWords, kBlockAlignWords) * 2u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint32_t off = (k * 32u + hl) * 16u;
    pre.words[k] = make_uint4(0, 0, 0, 0);
    if (off < paddedBytes) pre.words[k] = decLoad16(gwords + off);
  }
  pre.nc[0] = pre.nc[1] = typename Sink::GroupPre();
  if (wide) {
    pre.nc[0] = sink.prefetchGroup(kRowsPerBlock / 8u - 1u, hl);
    pre.nc[1] = sink.prefetchGroup(kRowsPerBlock / 8u - 2u, hl);
  }
}

// kTail (kFull): blocks that are NOT full -- the last block of an element, single-block elements of any size.  Only a
// block's LAST row can have lanes without a symbol, so the rows split into `topRows` rows at the top (the partial row,
// what is left of an incomplete 8-row group and -- two elements per wavefront -- the rows one half has and the other
// has not), decoded in groups of eight by the predicated step with one-word stores, and `groups` whole groups below
// them in which every lane of a half that has a block holds a symbol: those run the straight-line step with the wide
// stores.  `n` = symbols of this half's block (0 with kIdleUpper: the upper half has none).
template <int P, uint32_t FT, bool kFull, bool kWide = false, bool kIdleUpper = false, bool kCompact = false, bool kNoRing = false,
          bool kPre = false, bool kTail = false, typename Sink = RowSink<FT>>
__device__ __forceinline__ void decodeBlock(
    uint32_t xpose,                // kWide: LDS address of this half's transposition buffer
    uint32_t state,
    uint32_t n,                    // symbols in this half's block (0 = idle half)
    uint32_t groups,               // wave-uniform number of 8-row groups to run
    const uint8_t* __restrict__ gwords,  // global: this half's compressed words (16-byte aligned)
    uint32_t numWords,
    uint32_t ringBase,             // LDS address of this half's 2 KiB ring (multiple of 2048)
    const void* __restrict__ lutRaw, // LDS: uint2 entries, or uint32 entries (kCompact)
    const Sink& sink,              // RowSink<FT>, or AccumSink<FT>
    uint32_t hl,
    bool upper,
    const DecodePreOf<typename Sink::GroupPre>* pre = nullptr,  // kPre: the staging loads were issued by the caller (decodePrefetch)
    uint32_t topRows = 0) {          // kTail: rows above the `groups` whole groups (wave-uniform)
  static_assert(!kPre || (kNoRing && kFull), "");
  static_assert(!kTail || (kFull && !kPre), "");
  constexpr uint32_t kMask = (1u << P) - 1u;
  const uint32_t laneMaskLt = (1u << hl) - 1u;
  // LUT entry of slot x as {pdf | sym << 24, x - cdf} (the compact form is unpacked here)
  auto lutAt = [&](uint32_t x) -> uint2 {
    if (kCompact) {
      const uint32_t e = ((const uint32_t*)lutRaw)[x];
      return make_uint2((e & 0xff000fffu), (e >> 12) & 0xfffu);
    }
    return ((const uint2*)lutRaw)[x];
  };
  const uint32_t paddedBytes = roundUp(numWords, kBlockAlignWords) * 2u;

  // unread words of this half's block
  uint32_t posw = numWords;

  static_assert(!kNoRing || kFull, "whole-block staging is a full-block path");
  // initial fill: every chunk that intersects [numWords - 512, numWords)
  int lowChunk = numWords ? (int)((numWords - 1u) / kRingChunkWords) + 1 : 0;  // lowest chunk requested so far (+1 = none)
  if (kNoRing) {
    // the whole block (<= 1024 words = the 2 KiB ring region), word i at ringBase + 2 i
    uint4 v[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t off = (k * 32u + hl) * 16u;
      if (kPre) {
        v[k] = pre->words[k];
      } else {
        v[k] = make_uint4(0, 0, 0, 0);
        if (off < paddedBytes) v[k] = decLoad16(gwords + off);
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t off = (k * 32u + hl) * 16u;
      if (off < paddedBytes) *(LdsU4*)(uintptr_t)(ringBase + off) = u32x4{v[k].x, v[k].y, v[k].z, v[k].w};
    }
    lowChunk = 0;
  } else {
    const int stop = numWords > 512u ? (int)((numWords - 512u) / kRingChunkWords) : 0;
    while (lowChunk > stop) {
      --lowChunk;
      const uint32_t off = (uint32_t)lowChunk * 512u + hl * 16u;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (off < paddedBytes) v = decLoad16(gwords + off);
      *(LdsU4*)(uintptr_t)(ringBase | (((uint32_t)lowChunk & 3u) * 512u + hl * 16u)) = u32x4{v.x, v.y, v.z, v.w};
    }
  }
  uint4 pending = make_uint4(0, 0, 0, 0);
  int pendingChunk = -1;

  // Generic step (partial blocks): predicated, the word read under a branch.
  auto step = [&](bool valid) -> uint32_t {
    const uint2 e = lutAt(state & kMask);
    if (valid) state = __umul24(e.x, state >> P) + e.y;
    const bool read = valid && (state < kMinState);
    const uint64_t vote = __ballot(read);
    const uint32_t vh = upper ? (uint32_t)(vote >> 32) : (uint32_t)vote;
    posw -= __popc(vh);
    if (read) {
      // reading lanes take words from the top down in descending lane order:
      // word index = (new position) + number of reading lanes below me
      const uint32_t idx = posw + __popc(vh & laneMaskLt);
      const uint32_t w = *(const LdsU16*)(uintptr_t)(((idx << 1) & (kRingBytes - 1u)) | ringBase);
      state = (state << kEncodedBits) | w;
    }
    return e.x;
  };

  // Full-block step: straight-line code, no exec-mask change and no branch.
  // Every lane reads a ring word (the address always falls inside the ring); only
  // lanes that need to renormalise keep it.
  // wave-uniform positions (SGPRs): unread words of the lower / upper half's block; kNoRing: plus the LDS word
  // address of the block's staging area, so that (position + rank) << 1 IS the LDS address
  typedef typename Sink::Pre Pre;
  typedef typename Sink::GroupPre GroupPre;
  uint32_t sLo = 0, sHi = 0;
  // an idle upper half follows the lower half's addresses (in bounds; its words are never used)
  int upperSel = (upper && !kIdleUpper) ? 1 : 0;
  asm volatile("" : "+v"(upperSel));  // a VGPR operand of the multiply-add, not a select to be folded into it
  auto stepFull = [&]() -> uint32_t {
    const uint2 e = lutAt(state & kMask);
    state = __umul24(e.x, state >> P) + e.y;
    const bool read = state < kMinState;
    const uint64_t vote = __ballot(read);
    const uint32_t vLo = (uint32_t)vote, vHi = (uint32_t)(vote >> 32);
    const uint32_t sLoOld = sLo;
    sLo -= (uint32_t)__popc(vLo);
    sHi -= (uint32_t)__popc(vHi);
    // readers below me in the wave: lower half = my rank, upper half = rank + readers of the lower half
    uint32_t t = __builtin_amdgcn_mbcnt_hi(vHi, __builtin_amdgcn_mbcnt_lo(vLo, 0u));
    // lower: sLo + rank; upper: sHi + rank = sLo + (rank + readersLo) + (sHi - sLoOld)
    t = (uint32_t)(__mul24(upperSel, (int)(sHi - sLoOld)) + (int)t);
    asm volatile("" : "+v"(t));  // keep the scalar position in the add-shift below (one SGPR operand per VALU op)
    const uint32_t addr = kNoRing ? ((t + sLo) << 1) : ((((t + sLo) << 1) & (kRingBytes - 1u)) | ringBase);
    const uint32_t w = *(const LdsU16*)(uintptr_t)addr;
    state = read ? ((state << kEncodedBits) | w) : state;
    return e.x;
  };

  // Groups gHi .. gLo of the block, top down; F = every lane of a half that has a block holds a symbol in each of them
  // (the straight-line step, wide stores where the sink has them), else the predicated step with one-word stores.
  //
  // Non-compressed bytes are fetched ahead of their use: TWO groups on the wide path (a group takes ~1.5 us with three
  // workgroups per CU -- one group ahead did not cover the latency of HBM under load on cold buffers), one otherwise.
  //  * wide path: ONE 8-byte load per lane and group -- the 8 consecutive bytes that belong to the 8 consecutive
  //    words the lane stores; they meet the decoded symbols only at the flush (RowSink::flushGroup), so a row
  //    costs no VALU for the join and no byte load;
  //  * otherwise one byte load per row, unconditional (row index clamped) so that the compiler can use counted
  //    vmcnt waits instead of draining the memory queue every group.
  auto runGroups = [&](auto fullTag, const int gHi, const int gLo) {
    constexpr bool F = decltype(fullTag)::value;
    constexpr bool kJoinAtFlush = F && kWide;
    Pre preCur[kGroupRows], preNext[kGroupRows];
    GroupPre ncCur = GroupPre(), ncNext = GroupPre(), ncNext2 = GroupPre();
    if (kJoinAtFlush) {
      if (kPre) {
        ncCur = pre->nc[0];
        ncNext = pre->nc[1];
      } else {
        ncCur = sink.prefetchGroup((uint32_t)gHi, hl);
        ncNext = sink.prefetchGroup(gHi > gLo ? (uint32_t)(gHi - 1) : (uint32_t)gLo, hl);
      }
    }
#pragma unroll
    for (int j = 0; j < (int)kGroupRows; ++j) {
      const uint32_t row = (uint32_t)gHi * kGroupRows + j;
      preCur[j] = kJoinAtFlush ? (Pre)0 : ((F || row * 32u + hl < n) ? sink.prefetch(row) : (Pre)0);
    }

#pragma unroll 1
    for (int g = gHi; g >= gLo; --g) {
      const uint32_t gNext = g > gLo ? (uint32_t)(g - 1) : (uint32_t)gLo;
      if (kJoinAtFlush) {
        ncNext2 = sink.prefetchGroup(g > gLo + 1 ? (uint32_t)(g - 2) : (uint32_t)gLo, hl);
      } else {
#pragma unroll
        for (int j = 0; j < (int)kGroupRows; ++j) {
          const uint32_t row = gNext * kGroupRows + j;
          preNext[j] = (F || row * 32u + hl < n) ? sink.prefetch(row) : (Pre)0;
        }
      }
      // ring maintenance
      if (F && !kNoRing) posw = upper ? sHi : sLo;
      if (!kNoRing) {
        if (pendingChunk >= 0) {
          *(LdsU4*)(uintptr_t)(ringBase | (((uint32_t)pendingChunk & 3u) * 512u + hl * 16u)) = u32x4{pending.x, pending.y, pending.z, pending.w};
          pendingChunk = -1;
        }
        if (lowChunk > 0 && (uint32_t)lowChunk * kRingChunkWords + 512u > posw) {
          --lowChunk;
          const uint32_t off = (uint32_t)lowChunk * 512u + hl * 16u;
          pending = (off < paddedBytes) ? decLoad16(gwords + off) : make_uint4(0, 0, 0, 0);
          pendingChunk = lowChunk;
        }
      }
#pragma unroll
      for (int j = (int)kGroupRows - 1; j >= 0; --j) {
        const uint32_t row = (uint32_t)g * kGroupRows + j;
        if (F) {
          const uint32_t e0 = stepFull();
          if (kWide) {
            if (!kIdleUpper || !upper) sink.stageRow(xpose, (uint32_t)j, hl, e0);
          } else if (!kIdleUpper || !upper) {
            sink.store(row, e0, preCur[j]);
          }
        } else {
          const bool valid = row * 32u + hl < n;
          const uint32_t e0 = step(valid);
          if (valid) sink.store(row, e0, preCur[j]);
        }
      }
      if (kJoinAtFlush) {
        if (!kIdleUpper || !upper) sink.flushGroup(xpose, (uint32_t)g, hl, ncCur);
        ncCur = ncNext;
        ncNext = ncNext2;
      } else {
#pragma unroll
        for (int j = 0; j < (int)kGroupRows; ++j) preCur[j] = preNext[j];
      }
    }
  };

  if (kTail) {
    // the groups above the whole ones, predicated (see the comment at the template); the ring, where there is one, is
    // kept by the same per-group maintenance in both phases
    if (topRows != 0u) runGroups(std::false_type{}, (int)(groups + divUp(topRows, kGroupRows)) - 1, (int)groups);
    if (groups == 0u) return;  // uniform: the block had no whole group
  }
  if (kFull) {
    // wave-uniform positions (SGPRs): unread words of the lower / upper half's block (numWords, less what the groups
    // above consumed); kNoRing: plus the LDS word address of the block's staging area, so that (position + rank) << 1
    // IS the LDS address
    sLo = __builtin_amdgcn_readlane(posw, 0);
    sHi = __builtin_amdgcn_readlane(posw, 32);
    if (kNoRing) {
      sLo += __builtin_amdgcn_readlane(ringBase, 0) >> 1;
      sHi += __builtin_amdgcn_readlane(ringBase, 32) >> 1;
    }
  }
  runGroups(std::integral_constant<bool, kFull>{}, (int)groups - 1, 0);
}

// One workgroup of the tiled decoder: 32 threads per block of the tile (512 or 128), LDS = word rings + 64-bit LUT.
// The body of k_ans_decode (DecodeForm::kWhole), k_ans_decode_range (kRanged), k_ans_decode_accum (kAccum) and
// k_ans_decode_scaled (kWholeScaled), k_ans_decode_accum_scaled (kAccumScaled) and k_ans_decode_update (kUpdate), below.
//
// kRanged: blocks [firstBlock[b], firstBlock[b] + numBlocks[b]) of element b, clipped to the element's end, and block
// firstBlock + k goes to out + k * 4096 words: the output buffer holds the range, not the element.
//   * Tiles are counted from the range's first block (half-wave hw of tile t has block firstBlock + t * kTileBlocks + hw),
//     so the waves of a range are filled from the bottom whatever the parity of firstBlock, every wave but the last holds
//     two full blocks, and the work list (always kDecOrderMap) has ceil(blocks of the range / kTileBlocks) tiles per
//     element.  Blocks past the range's end behave like blocks past the element's end: not fetched, decoded or stored.
//   * Tile 0 of the list reports the element and vouches for the descriptors OF THE RANGE only: a corrupt descriptor
//     outside the range is neither read nor noticed, and does not affect the call.  The cost follows the range.
//   * Header checks as for the whole element (magic, version, probBits, float type, block count, pdf sum, the archive
//     inside inBytes); success also needs firstBlock * 4096 <= total (a range that begins exactly at the end is empty
//     and succeeds) and the clipped range inside the capacity.  outSize = words (bytes) of the clipped range.  The
//     capacity is that of the range buffer, so it does not bound the element's size; inBytes (always given) does.
//   * Read from the archive: the headers, the pdf table, descriptors, lane states and compressed words of the range's
//     blocks and their slices of the non-compressed plane(s).  A checksum in the archive is ignored.
//   * An element with numBlocks == 0 has no tile; workgroup 0 of the grid reports it (size 0, success) without reading
//     its archive.  A call of nothing but such elements lists one entry whose element index is not below numInBatch.
//
// kAccum: a whole bounded decode whose words are widened to float32 and stored to / added into the float32 accumulator
// a.out.ptr(b) (AccumSink; capacities in float words; float types only).  Row loop, ring, LUT build, checks, success and
// outSize are those of the whole decode, with one difference: EVERY tile makes tile 0's check of all the element's block
// descriptors (8 bytes per block, from the L2, in the round trip of the tile's own descriptor), and no tile of an element
// with a malformed descriptor stores -- a failing element leaves its accumulator as it was.
//
// kWholeScaled: the whole bounded decode of a float archive whose every word is multiplied by the member's float32 factor
// and rounded back to FT before it is stored (ScaledSink).  Everything else -- checks, success, outSize, the words behind
// a short element -- is kWhole's.  The factor (DecodeArgs::scalePtr / scaleStride, or the host's DecodeArgs::scale) is
// wave-uniform and is requested with the header, so it is there long before the first store.
//
// kAccumScaled: kAccum whose widened word is multiplied by the member's float32 factor before it is stored or added:
// acc = [acc +] fl32(widened * factor), one multiply and one add, never fused (AccumSink, kPreScaled).  The factor is
// fetched as kWholeScaled fetches it; everything else is kAccum's, the descriptor checks of every tile included.
//
// kUpdate: the factor of kAccumScaled, the 16-bit output of kWholeScaled: out = sround_FT([widen(out) +] fl32(widened *
// factor)) (UpdateSink; float16 and bfloat16 only).  Checks, success and outSize are kAccum's, the descriptor checks of
// every tile included: a failing member keeps every bit of its tensor.  The seed (DecodeArgs::seedPtr, or the host's
// DecodeArgs::seed) is requested with the factor, in the round trip of the header; the member's key follows from it in
// scalar registers, once per tile.
// (kReduce: decodeReduceTile, below)
enum class DecodeForm { kWhole, kRanged, kAccum, kReduce, kReduceStats, kReduceMixed, kReduceMixedStats, kReduceScaled, kReduceScaledStats, kReduceNorm, kReduceNormStats, kWholeScaled, kAccumScaled, kUpdate };
template <int P, uint32_t FT, uint32_t kTileBlocks, DecodeForm kForm>
__device__ __forceinline__ void decodeTile(const DecodeArgs& a) {
  constexpr bool kRanged = kForm == DecodeForm::kRanged, kAccumScaled = kForm == DecodeForm::kAccumScaled;
  constexpr bool kUpdate = kForm == DecodeForm::kUpdate;
  constexpr bool kAccum = kForm == DecodeForm::kAccum || kAccumScaled || kUpdate;      // the accumulating forms
  constexpr bool kScaledForm = kForm == DecodeForm::kWholeScaled || kAccumScaled || kUpdate;  // the forms with a factor
  static_assert(kForm == DecodeForm::kWhole || kForm == DecodeForm::kRanged || kAccum || kScaledForm,
                "decode-reduce has a body of its own: decodeReduceTile");
  static_assert(!(kAccum || kScaledForm) || FT != 0u, "accumulating and scaled decode: float archives only");
  static_assert(!kUpdate || FT == kFloat16 || FT == kBFloat16, "decode-update: 16-bit float archives only");
  using Sink = std::conditional_t<kUpdate, UpdateSink<kUpdate ? FT : kBFloat16>,
                                  std::conditional_t<kAccum, AccumSink<FT ? FT : kFloat32, 0u, false, false, kAccumScaled>,
                                                     std::conditional_t<kScaledForm, ScaledSink<FT ? FT : kFloat32>, RowSink<FT>>>>;
  constexpr uint32_t kDecThreads = decThreads(kTileBlocks);
  // the LUT-build scratch (cdf, pdf: 2 KiB, read while the LUT is stored) sits in the ring area
  static_assert(kTileBlocks * kRingBytes >= 2048u, "");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  // rings: 16 x 2 KiB at LDS offset 0 (2 KiB aligned), then the LUT, then the transposition buffers
  uint2* sLut = (uint2*)(smem + kTileBlocks * kRingBytes);
  constexpr uint32_t kXpose = decXposeBytes(P, FT, kTileBlocks);

  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = tid >> 6;
  const bool upper = lane >= 32u;
  const uint32_t hl = lane & 31u;
  const uint32_t hw = wave * 2u + (upper ? 1u : 0u);
  uint32_t b, tile;
  if (!decodeTileOf(a, blockIdx.x, &b, &tile)) return;  // uniform (kDecOrderXcd pads the grid to a multiple of 8 elements)
  uint32_t rFirst = 0;   // kRanged: first block of the range
  uint64_t rEnd = 0;     // kRanged: one past its last block, as requested (not yet clipped to the element)
  if constexpr (kRanged) {
    if (blockIdx.x == 0) {
      for (uint32_t e = tid; e < a.numInBatch; e += kDecThreads) {
        if (a.numBlocks[e] == 0u) {
          if (a.outSuccess) a.outSuccess[e] = 1;
          if (a.outSize) a.outSize[e] = 0;
        }
      }
    }
    if (b >= a.numInBatch) return;  // uniform: the entry of a list without tiles
    rFirst = a.firstBlock[b];
    rEnd = (uint64_t)rFirst + a.numBlocks[b];
  }
  // kRanged: words (bytes) of the range in an element of `total`; 0 for a range that begins past the end
  auto rangeWords = [&](uint32_t total) -> uint32_t {
    const uint64_t lo = (uint64_t)rFirst * kBlockSize, hi = rEnd * kBlockSize;
    return lo > total ? 0u : (uint32_t)((hi < total ? hi : (uint64_t)total) - lo);
  };

  const uint8_t* archive = a.in.ptr(b);
  uint32_t floatSize = 0;
  const uint64_t inBytes = decodeInBytes(a, b);
  if (inBytes < (FT ? sizeof(FloatHeader) : sizeof(AnsHeader))) {  // uniform: not even a header
    if (tile == 0 && tid == 0) {
      if (a.outSuccess) a.outSuccess[b] = 0;
      if (a.outSize) a.outSize[b] = 0;
    }
    return;
  }
  if (FT) {
    // the float header locates the ANS archive: check it before following it
    // (GpuFloatHeader::checkMagicAndVersion / getFloatType asserts, GpuFloatUtils.cuh:31-41, GpuFloatDecompress.cuh:332-382)
    const FloatHeader fh = *(const FloatHeader*)archive;
    // (kRanged: the capacity is the range's and is checked against the range below)
    const bool fhOk = fh.magicAndVersion == ((kFloatMagic << 16) | kFloatVersion) && (fh.options & 0xfu) == FT &&
        (kRanged || fh.size <= a.out.size(b)) &&
        (uint64_t)sizeof(FloatHeader) + floatUncompDataSize(FT, fh.size) + sizeof(AnsHeader) <= inBytes;
    if (!fhOk) {  // uniform
      if (tile == 0 && tid == 0) {
        if (a.outSuccess) a.outSuccess[b] = 0;
        if (a.outSize) a.outSize[b] = kRanged ? rangeWords(fh.size) : fh.size;
      }
      return;
    }
  }
  const uint8_t* ans = locateAns(archive, FT, &floatSize);
  // Everything at an offset from the ANS archive that is known NOW is requested in one round trip with the header:
  // the pdf table (wave 0) and -- float archives: a valid one holds ceil(size / 4096) blocks, which the header check
  // below confirms -- this half-wave's block descriptor and lane states.  A part is requested early only where it is
  // known to lie inside the caller's buffer: the caller said how many bytes there are, or (archives of unknown extent)
  // a checked float header says that an ANS archive of that many blocks follows.  Raw ANS archives learn their block
  // count from the header and fetch descriptor and states after it, as before.  A load that is not to be made yet
  // reads the first bytes of the header again.
  uint32_t block = tile * kTileBlocks + hw;
  bool inRange = true;
  if constexpr (kRanged) {
    const uint64_t blk = (uint64_t)rFirst + block;
    inRange = blk < rEnd;
    block = inRange ? (uint32_t)blk : 0u;
  }
  const bool extentKnown = inBytes != ~0ull;
  const uint32_t ansOff = ansOffsetInArchive(FT, floatSize);
  const uint32_t nbSpec = FT ? divUp(floatSize, kBlockSize) : 0u;
  const bool pdfEarly = extentKnown ? (uint64_t)ansOff + ansOverhead(0u) <= inBytes : FT != 0u;
  const bool blockEarly = FT != 0u && inRange && block < nbSpec && (!extentKnown || (uint64_t)ansOff + ansOverhead(nbSpec) <= inBytes);
  const AnsHeader header = *(const AnsHeader*)ans;
  float factor = 1.0f;  // kScaledForm: the member's factor, in the round trip of the header
  if constexpr (kScaledForm) factor = a.scalePtr ? a.scalePtr[(size_t)b * a.scaleStride] : a.scale;
  uint64_t seed = 0;    // kUpdate: the call's seed, in the same round trip
  if constexpr (kUpdate) seed = a.seedPtr ? *a.seedPtr : a.seed;
  uint2 pdfRaw = make_uint2(0u, 0u);
  if (wave == 0) pdfRaw = *(const uint2*)(pdfEarly ? ans + sizeof(AnsHeader) + 8u * lane : ans);  // pdf[4 lane .. 4 lane + 3]
  uint2 bwMine = *(const uint2*)(blockEarly ? ans + ansBlockWordsOffset(nbSpec) + 8u * block : ans);
  uint32_t state = *(const uint32_t*)(blockEarly ? ans + ansStatesOffset() + 4u * (block * 32u + hl) : ans);
  const uint32_t nb = header.numBlocks;
  const uint32_t total = header.totalUncompressedWords;
  const uint32_t totalWords = header.totalCompressedWords;

  // Is there room for the output?  Capacity and size are in the API's units
  // (bytes for raw ANS, float words for the float codec); GpuANSDecode.cuh:325-341.
  // The format invariants the reference only asserts (GpuANSDecode.cuh:323,448,
  // GpuANSUtils.cuh:109-112) are CHECKED here: a corrupt or truncated archive is
  // reported through outSuccess instead of being followed out of bounds.  Every
  // quantity used for addressing below is bounded by the caller's capacity:
  // total <= capacity, nb == ceil(total / 4096), block sizes as the format
  // prescribes, block data inside [0, totalCompressedWords).
  bool success = a.out.size(b) >= total;
  if constexpr (kRanged) success = (uint64_t)rFirst * kBlockSize <= total && rangeWords(total) <= a.out.size(b);
  success = success && header.magicAndVersion == ((kAnsMagic << 16) | kAnsVersion) &&
      (header.options & 0xfu) == (uint32_t)P;
  if (FT) success = success && floatSize == total;
  success = success && nb == divUp(total, kBlockSize);
  // the archive as a whole fits the bytes the caller has (when told)
  success = success && (uint64_t)ansOffsetInArchive(FT, total) + ansOverhead(nb) + 2ull * totalWords <= inBytes;
  if (!success) {  // uniform: nothing else of the archive is read
    if (tile == 0 && tid == 0) {
      if (a.outSuccess) a.outSuccess[b] = 0;
      if (a.outSize) a.outSize[b] = kRanged ? rangeWords(total) : total;
    }
    return;
  }
  // the blocks this workgroup may touch: [.., endBlock), and the first one of its tile
  uint32_t endBlock = nb, tileFirst = tile * kTileBlocks;
  if constexpr (kRanged) {
    endBlock = rEnd < nb ? (uint32_t)rEnd : nb;  // (rFirst <= nb: the range begins inside the element)
    tileFirst += rFirst;
  }
  if (tileFirst >= endBlock && tile != 0) return;

  const uint2* blockWords = (const uint2*)(ans + ansBlockWordsOffset(nb));
  // {uncompressed words << 16 | compressed words, start} of block i must be what an
  // encoder can produce: the size the format prescribes, 16-byte aligned data inside the archive
  auto blockOk = [&](uint32_t i, uint2 bw) -> bool {
    const uint32_t want = (i + 1u < nb) ? kBlockSize : total - i * kBlockSize;
    const uint32_t words = bw.x & 0xffffu;
    return (bw.x >> 16) == want && (bw.y & (kBlockAlignWords - 1u)) == 0u &&
        (uint64_t)bw.y + roundUp(words, kBlockAlignWords) <= (uint64_t)totalWords;
  };
  // tile 0 vouches for the whole element (kRanged: the whole range; it alone writes outSuccess); its loads are
  // issued here and checked after the LUT build
  bool allBlocksOk = true;
  if constexpr (kAccum) {
    // every tile vouches for the whole element (see above); the loads do not wait for each other
    for (uint32_t i = tid; i < endBlock; i += kDecThreads) allBlocksOk = blockOk(i, blockWords[i]) & allBlocksOk;
  } else if (tile == 0) {
    for (uint32_t i = rFirst + tid; i < endBlock; i += kDecThreads) allBlocksOk = allBlocksOk && blockOk(i, blockWords[i]);
  }

  // This half-wave's block descriptor and lane states and (wave 0) the pdf table: already on their way (float
  // archives, above), or requested NOW, in the same round trip as tile 0's descriptor checks; as soon as the descriptor
  // is there the block's compressed words and its first non-compressed bytes are requested too (decodePrefetch), and
  // all of it lands while the LUT is being built.
  bool haveBlock = inRange && block < endBlock;
  if (!haveBlock) {
    bwMine = make_uint2(0u, 0u);
    state = 0;
  } else if (!blockEarly) {  // (for a float archive the checked header has confirmed nb == nbSpec)
    bwMine = blockWords[block];
    state = ((const uint32_t*)(ans + ansStatesOffset()))[block * 32u + hl];  // (inside the archive: nb was checked against inBytes)
  }
  if (wave == 0 && !pdfEarly) pdfRaw = ((const uint2*)(ans + sizeof(AnsHeader)))[lane];
  uint32_t n = 0, numWords = 0, start = 0;
  if (haveBlock) {
    if (blockOk(block, bwMine)) {
      n = bwMine.x >> 16;
      numWords = bwMine.x & 0xffffu;
      start = bwMine.y;
    } else {
      haveBlock = false;  // malformed block: neither read nor written (tile 0 reports the element)
      state = 0;
    }
  }
  const uint8_t* gwords = ans + ansOverhead(nb) + 2u * (size_t)start;
  Sink sink;
  if constexpr (kAccum) sink.accumulate = a.accumulate;
  if constexpr (kAccumScaled) sink.preFactor = factor;
  else if constexpr (kScaledForm) sink.factor = factor;
  if constexpr (kUpdate) sink.key = srMemberKey(seed, a.firstMember + b);
  // (a half without a block points at its wave's first block: its prefetches must stay inside the archive -- kAccum:
  // and inside the accumulator)
  uint32_t sinkBlock = haveBlock ? block : (block & ~1u);
  if constexpr (kRanged) sinkBlock = haveBlock ? block : tileFirst + (hw & ~1u);
  sink.init(a.out.ptr(b), archive, floatSize, (size_t)sinkBlock * kBlockSize, hl);
  if constexpr (kRanged) sink.out -= (size_t)rFirst * kBlockSize;  // the planes are the element's, the output is the range's
  // LDS address of the dynamic segment (0: this kernel has no static LDS); the
  // rings must be 2 KiB aligned for the and-or addressing in decodeBlock
  const uint32_t ldsBase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem;
  // uniform per wave: both halves hold full blocks?  small enough to be staged whole?
  const uint32_t nFirst = __shfl(n, 0, 64);
  const uint32_t nSecond = __shfl(n, 32, 64);
  const uint32_t wFirst = __shfl(numWords, 0, 64);
  const uint32_t wSecond = __shfl(numWords, 32, 64);
  const bool noRing = wFirst <= kRingBytes / 2u && wSecond <= kRingBytes / 2u;
  // (the wide stores cover whole 8-row groups of words that exist; they take any word-aligned output element)
  // (kAccum: accumulators are float-aligned, the host checks it)
  const bool wide = decXposeBytes(P, FT, kTileBlocks) != 0 && (kAccum || (((uintptr_t)a.out.ptr(b)) & (decOutWordBytes(FT) - 1u)) == 0);
  const bool fullPair = nFirst == kBlockSize && nSecond == kBlockSize;
  // one full block in the wave (odd block counts): fast path with an idle upper half
  const bool fullSingle = nFirst == kBlockSize && nSecond == 0u;
  DecodePreOf<typename Sink::GroupPre> pre;
  if ((fullPair || fullSingle) && noRing) decodePrefetch<FT>(pre, gwords, numWords, sink, hl, wide);

  // Decode LUT, built by the workgroup itself from the archive's pdf table (no
  // separate table kernel / LUT round trip through HBM):
  //   lut[x] = { pdf[sym] | sym << 24,  x - cdf[sym] },  sym = symbol whose cdf range holds x
  // (the information of packDecodeLookup, GpuANSDecode.cuh:34-41, re-packed so
  // that v_mad_u32_u24 can take word 0 directly: its low 24 bits are the pdf).
  // Wave 0 scans the 256 pdfs on its own (4 per lane), so one barrier suffices;
  // the cdf/pdf scratch lives in the ring area, which is not in use yet.
  uint32_t* sCdf = (uint32_t*)smem;
  uint32_t* sPdf = sCdf + kNumSymbols;
  uint32_t* sPdfSum = sPdf + kNumSymbols;
  uint32_t* sWaveBad = sPdfSum + 1;  // one flag per wave (<= 8); no static LDS in this kernel (ring alignment)
  // small tiles (one LUT per 4 blocks): the LUT is filled by a max-scan over symbol marks instead of a
  // binary search per slot (see below)
  constexpr bool kScanLut = kTileBlocks <= kDecBlocksPerSmallTile;
  uint32_t* sWaveTop = sWaveBad + 8;                  // kScanLut: running maximum at the end of each wave
  // kScanLut: 2^P mark bytes in the TAIL of the LUT region -- every mark has been read (into registers) before the
  // barrier that precedes the first LUT store
  constexpr bool kCompact = decCompactLut(P, kTileBlocks);
  constexpr uint32_t kLutBytes = decLutBytes(P, kTileBlocks);
  uint8_t* sMark = (uint8_t*)sLut + kLutBytes - (1u << P);
  {
    {
      const bool waveBad = __ballot(!allBlocksOk) != 0ull;
      if (lane == 0u) sWaveBad[wave] = waveBad ? 1u : 0u;
    }
    if (kScanLut) {
      for (uint32_t i = tid; i < (1u << P) / 4u; i += kDecThreads) ((uint32_t*)sMark)[i] = 0u;
    }
    if (wave == 0) {
      const uint2 raw = pdfRaw;
      const uint32_t p0 = raw.x & 0xffffu, p1 = raw.x >> 16, p2 = raw.y & 0xffffu, p3 = raw.y >> 16;
      const uint32_t mine = p0 + p1 + p2 + p3;
      const uint32_t incl = waveInclusiveScan(mine, lane);
      const uint32_t base = incl - mine;
      ((uint4*)sCdf)[lane] = make_uint4(base, base + p0, base + p0 + p1, base + p0 + p1 + p2);
      ((uint4*)sPdf)[lane] = make_uint4(p0, p1, p2, p3);
      if (lane == 63u) *sPdfSum = incl;
    }
    __syncthreads();
    // the reduction of tile 0's block checks
    uint32_t anyBad = 0;
#pragma unroll
    for (uint32_t w = 0; w < kDecThreads / 64u; ++w) anyBad |= sWaveBad[w];
    const bool blocksOk = anyBad == 0u;
    // the probabilities of a non-empty element sum to 2^P (GpuANSStatistics.cuh:256-316)
    const bool pdfOk = nb == 0u || *sPdfSum == (1u << P);
    if (tile == 0 && tid == 0) {
      if (a.outSuccess) a.outSuccess[b] = (blocksOk && pdfOk) ? 1 : 0;
      if (a.outSize) a.outSize[b] = kRanged ? rangeWords(total) : total;
    }
    if (!pdfOk || tileFirst >= endBlock) return;  // uniform
    if constexpr (kAccum) {
      if (!blocksOk) return;  // uniform
    }
    if constexpr (kScanLut) {
      // mark[cdf[s]] = s for every present symbol; sym(x) = the largest mark at or below x (cdfs ascend with
      // the symbol; slot 0 belongs to the first present symbol, so "no mark" = 0 never surfaces)
      for (uint32_t sidx = tid; sidx < kNumSymbols; sidx += kDecThreads) {
        if (sPdf[sidx]) sMark[sCdf[sidx]] = (uint8_t)sidx;
      }
      __syncthreads();
      // Every wave owns a contiguous part of the table and walks it 256 slots per step: a lane reads ONE dword of
      // marks (four consecutive slots) and writes ONE 16-byte vector of compact entries, both at consecutive
      // addresses across the lanes -- (1 << P) / threads CONSECUTIVE slots per thread meant 8 ... 16 entry stores at an
      // 8 ... 16-dword stride, i.e. that many lanes per LDS bank (the conflict k_ans_decode_pair's build had: section 4.4).
      // All marks are in registers before the barrier that precedes the first entry store (they live in the LUT's tail).
      static_assert(kCompact, "the scan build writes compact entries");
      constexpr uint32_t kWaves = kDecThreads / 64u;
      constexpr uint32_t kPart = (1u << P) / kWaves;  // slots per wave
      static_assert(kPart % 256u == 0u, "");
      constexpr uint32_t kSteps = kPart / 256u;
      auto dmax = [](uint32_t v, uint32_t o) { return v > o ? v : o; };
      auto waveMaxScan = [&](uint32_t v) -> uint32_t {  // inclusive, DPP
        v = dmax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
        v = dmax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
        v = dmax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
        v = dmax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
        v = dmax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true));
        v = dmax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true));
        return v;
      };
      uint32_t m4[kSteps];
      uint32_t top = 0;
#pragma unroll
      for (uint32_t t = 0; t < kSteps; ++t) {
        m4[t] = ((const uint32_t*)sMark)[(wave * kPart + t * 256u) / 4u + lane];
        const uint32_t a01 = dmax(m4[t] & 0xffu, (m4[t] >> 8) & 0xffu);
        const uint32_t a23 = dmax((m4[t] >> 16) & 0xffu, m4[t] >> 24);
        top = dmax(top, dmax(a01, a23));
      }
      top = waveMaxScan(top);
      if (lane == 63u) sWaveTop[wave] = top;  // the largest mark of this wave's part
      __syncthreads();
      uint32_t carry = 0;  // the largest mark before the step (uniform)
      for (uint32_t w = 0; w < wave; ++w) carry = dmax(carry, sWaveTop[w]);
#pragma unroll
      for (uint32_t t = 0; t < kSteps; ++t) {
        uint32_t run[4];
        run[0] = m4[t] & 0xffu;
        run[1] = dmax(run[0], (m4[t] >> 8) & 0xffu);
        run[2] = dmax(run[1], (m4[t] >> 16) & 0xffu);
        run[3] = dmax(run[2], m4[t] >> 24);
        const uint32_t incl = waveMaxScan(run[3]);
        uint32_t excl = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x138, 0xf, 0xf, true);  // wave_shr:1 (lane 0: 0)
        excl = dmax(excl, carry);
        uint32_t e[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
          const uint32_t x = wave * kPart + t * 256u + lane * 4u + j;
          const uint32_t sym = dmax(run[j], excl);
          e[j] = (sPdf[sym] & 0xfffu) | (((x - sCdf[sym]) & 0xfffu) << 12) | (sym << 24);
        }
        ((uint4*)sLut)[(wave * kPart + t * 256u) / 4u + lane] = make_uint4(e[0], e[1], e[2], e[3]);
        carry = dmax(carry, (uint32_t)__builtin_amdgcn_readlane((int)incl, 63));
      }
    } else
    for (uint32_t x = tid; x < (1u << P); x += kDecThreads) {
      // last symbol s with cdf[s] <= x (zero-pdf symbols share the cdf of their
      // successor and are skipped by taking the last one)
      uint32_t lo = 0, hi = kNumSymbols;  // invariant: cdf[lo] <= x, answer in [lo, hi)
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const uint32_t mid = (lo + hi) >> 1;
        const bool le = sCdf[mid] <= x;
        lo = le ? mid : lo;
        hi = le ? hi : mid;
      }
      if (kCompact) ((uint32_t*)sLut)[x] = (sPdf[lo] & 0xfffu) | (((x - sCdf[lo]) & 0xfffu) << 12) | (lo << 24);
      else sLut[x] = make_uint2((sPdf[lo] & 0xfffu) | (lo << 24), (x - sCdf[lo]) & 0xfffu);
    }
  }

  __syncthreads();  // LUT visible to every wave, scratch free (each half-wave's ring is private to its wave)

  constexpr uint32_t kLutBytesHere = decLutBytes(P, kTileBlocks);
  const uint32_t xpose = ldsBase + kTileBlocks * kRingBytes + kLutBytesHere + hw * kXpose;
  const uint32_t ringLds = ldsBase + hw * kRingBytes;
#define DGPU_DECODE_FULL(WIDE, IDLE, NORING) \
  decodeBlock<P, FT, true, WIDE, IDLE, kCompact, NORING, NORING>(xpose, state, n, kRowsPerBlock / kGroupRows, gwords, numWords, ringLds, sLut, sink, hl, upper, &pre)
  if (fullPair) {
    if (wide) {
      if (noRing) DGPU_DECODE_FULL(true, false, true); else DGPU_DECODE_FULL(true, false, false);
    } else {
      if (noRing) DGPU_DECODE_FULL(false, false, true); else DGPU_DECODE_FULL(false, false, false);
    }
  } else if (fullSingle) {
    if (wide) {
      if (noRing) DGPU_DECODE_FULL(true, true, true); else DGPU_DECODE_FULL(true, true, false);
    } else {
      if (noRing) DGPU_DECODE_FULL(false, true, true); else DGPU_DECODE_FULL(false, true, false);
    }
#undef DGPU_DECODE_FULL
  } else {
    // A wavefront with a block that is not full -- the element's last: (full, partial) or (partial, none).  The whole
    // 8-row groups in which every lane of a half that has a block holds a symbol run the straight-line step, the rows
    // above them the predicated one (decodeBlock, kTail); in ring mode only if those rows fit the ring's initial fill.
    const uint32_t maxN = nFirst > nSecond ? nFirst : nSecond;
    const uint32_t maxRows = divUp(maxN, 32u);
    const uint32_t fullRows = (nSecond ? nSecond : nFirst) / 32u;  // (the last block of the wave is the partial one)
    const uint32_t groups = fullRows / kGroupRows;
    const uint32_t topRows = maxRows - groups * kGroupRows;
    const bool tailPair = nFirst == kBlockSize && nSecond != 0u, tailSingle = nFirst != 0u && nSecond == 0u;
    if ((tailPair || tailSingle) && groups != 0u) {
#define DGPU_DECODE_TAIL(WIDE, IDLE, NORING) \
  decodeBlock<P, FT, true, WIDE, IDLE, kCompact, NORING, false, true>(xpose, state, n, groups, gwords, numWords, ringLds, sLut, sink, hl, upper, nullptr, topRows)
      if (tailPair) {
        if (wide) {
          if (noRing) DGPU_DECODE_TAIL(true, false, true); else DGPU_DECODE_TAIL(true, false, false);
        } else {
          if (noRing) DGPU_DECODE_TAIL(false, false, true); else DGPU_DECODE_TAIL(false, false, false);
        }
      } else {
        if (wide) {
          if (noRing) DGPU_DECODE_TAIL(true, true, true); else DGPU_DECODE_TAIL(true, true, false);
        } else {
          if (noRing) DGPU_DECODE_TAIL(false, true, true); else DGPU_DECODE_TAIL(false, true, false);
        }
      }
#undef DGPU_DECODE_TAIL
    } else {
      decodeBlock<P, FT, false, false, false, kCompact>(xpose, state, n, divUp(maxRows, kGroupRows), gwords, numWords, ringLds, sLut, sink, hl, upper);
    }
  }
}

// ---------------------------------------------------------------------------
// Decode-reduce (k_ans_decode_reduce): member b has S = numSources archives, in.ptr(b * S + s), and ONE float32
// accumulator; the workgroup of (member, tile) decodes its blocks of source 0, 1, ... S-1 one after the other into the
// accumulator words of the tile -- acc = ((acc + x0) + x1) + ..., or (x0 + x1) + ... with accumulate == 0 -- which is bit for
// bit what S decode-accumulate calls leave.  Grid, workgroup order, tile-to-block mapping, LDS layout, sink and row loop
// (decodeBlock) are k_ans_decode_accum's.  A sibling of decodeTile, not a form of it: that function is the body of
// every shipped decoder and stays as it is.
//
// 1. ALL sources are validated before the first store, in every tile of the member, so a member with one bad source
//    keeps every bit of its accumulator.  Wave w checks the headers (those of a bounded decode-accumulate against the
//    member's capacity and the source's own inBytes) and sums the pdf table of sources w, w + waves, ...; after a barrier
//    every thread knows the S verdicts and word counts, which must all be equal; then the S * numBlocks block descriptors
//    are checked in ONE strided loop over the workgroup (8 bytes each, from the L2, no load waiting for another), and a
//    second barrier collects that verdict.  Tile 0 reports: success, and the word count source 0 states.
// 2. Per source: descriptor, lane states and (wave 0) pdf table are requested; the LUT is rebuilt (the binary-search
//    build for both tile sizes: the scan build of the small tiles would be a second copy of sixty lines for a
//    start-up cost that a tile pays once per source); decodeBlock runs with accumulate = (s > 0) | a.accumulate.
//    Between two sources the accumulator goes through memory: the words a wave adds to for source s + 1 are the words
//    the same wave stored for source s, though other lanes may have (wide layout).  So before the barrier that frees
//    rings and LUT for the rebuild every wave releases at workgroup scope and drains its stores; after it, it acquires,
//    and only then are the accumulator words of source s + 1 requested (decodePrefetch and everything in decodeBlock).
//    The workgroup sits on one CU, whose L1 all its waves share: this costs the wait and no cache invalidation.
//
// kStats (k_ans_decode_reduce_stats, the first half of reduce-compress): the same, and on the LAST source the sink counts
// the exponent byte of every sum it stores, rounded to FT as the cast encoder will round it (AccumSink, kSlots), in LDS
// bins behind the store buffers -- the histogram kernel's bin-major layout, decStatsSlots lane slots per bin, zeroed
// before the first barrier.  When the tile is done the workgroup folds its bins and adds the non-zero ones to the
// member's 256 counters a.stats[b] with relaxed agent-scope atomics.  A member's sources must state EXACTLY its capacity
// (the encoder codes `capacity` words of the accumulator); a member that fails any check returns before the source loop
// and so adds nothing.  The last source is selected at run time (a wave-uniform test around the counting), the form at
// compile time: the plain kernel's code does not change.
//
// kMixed (k_ans_decode_reduce_mixed, k_ans_decode_reduce_mixed_stats): a source is an archive or a RAW row of
// inBytes / wordBytes words of FT, added in its place in source order.  The kind travels in the source's address in the
// parameter block: a raw row's has bit 0 set (kReduceRawTag; the host checks that rows are word-aligned and archives
// 16-byte aligned, so the bit is free) -- the address is loaded anyway, where a separate array of kinds is two more
// live scalars, one more than the counting bf16 form has (it then keeps one in a VGPR lane: 129 VGPRs).  A raw row's
// verdict needs no header: the count it states is its total and what it reports, and must fit the capacity (kStats:
// equal it) like a header's; it has no block descriptors and no pdf.  In the source loop it takes its turn before
// anything of the archive path is set up (reduceRawSource: in one block with that path its values stretch the live
// ranges across decodeBlock, 167 VGPRs): the same hand-over barrier, the same sink, and instead of LUT build and
// decodeBlock every half-wave streams its own block's words into the sink (reduceRawBlock) -- in the sink's own
// lane-to-word mapping, so a lane touches the accumulator words it touches for an archive source, and the hand-over
// holds in both directions.  No LDS is used, so nothing of it races with the builds of the sources around it.  Kind
// and base alignment are uniform per source; the form is a template flag: the plain and counting kernels do not change.
//
// kScaled (the *_scaled kernels, built for the mixed forms, which take all-archive members as well): the last source's
// store leaves fl32(sum * a.scale) instead of the sum, and the counting form counts that product (AccumSink, kScaled).
// The factor is a kernel argument, not part of the parameter block: calls that differ in it alone share the block.  The
// counting form writes it behind the bins, one float per slot column, when it zeroes them.  A template flag again: every
// unscaled kernel keeps its code, and scale 1 launches those.
//
// kNorm (the *_norm kernels, forms of the scaled ones that also take a factor of 1): when the last source is in the
// accumulator the workgroup MEASURES the words it left there -- the words of this tile that the sources state, read back
// through the hand-over that every source change uses, right behind the (non-temporal) stores that left them and not
// in a later pass over the whole shard; which level of the memory system serves that read has not been measured.
// (Measuring inside the sinks, in the registers the words are stored from, does not
// fit: the counting 16-bit form has 128 VGPRs and the scalar file full, and a float64 partial in a per-lane LDS slot
// beside each store still costs it 3 to 5 VGPRs and a dozen spilled scalars: three waves per SIMD for every pass.)
// The measured word is the float32 word itself, or in the counting form that word rounded to FT by castRound and widened
// again: the word of the archive the cast encoder will write, where a finite float32 sum may have become an infinity.
// A finite measured word adds its square to the thread's float64 partial -- the square of a widened float32 is exact, so
// the only rounding is the add's -- and any other adds one to the thread's count.  Thread t takes the 16-byte quads t,
// t + threads, ... of the tile in that order; the partials are added in a fixed tree over the lanes of a wave and then in
// wave order, and leave as one float64 and one count per (member, tile) with plain stores: the same bits every time,
// whichever workgroup ran the tile.  A workgroup that returns before the source loop -- a failed member, a tile past the
// member's end -- stores nothing: the host zeroes the slots before the launch.
template <uint32_t FT, bool kRounded>
__device__ __forceinline__ uint32_t normWord(uint32_t o) {  // the float32 bits of the word measured for the stored bits o
  if constexpr (!kRounded) {
    return o;
  } else if constexpr (FT == kBFloat16) {
    return castRoundHigh<kBFloat16>(o) & 0xffff0000u;
  } else {
    return __builtin_bit_cast(uint32_t, accWiden16<kFloat16>(castRound<kFloat16>(o)));
  }
}
template <uint32_t FT, bool kRounded>
__device__ __forceinline__ void normMeasure(uint32_t o, double& sq, uint32_t& bad) {
  const uint32_t m = normWord<FT, kRounded>(o);
  const bool finite = (m & 0x7f800000u) != 0x7f800000u;
  const double d = (double)__builtin_bit_cast(float, finite ? m : 0u);
  sq = __fma_rn(d, d, sq);
  bad += finite ? 0u : 1u;
}
__device__ __forceinline__ void reduceHandOver();
// What the measuring pass of a tile needs, written to LDS by thread 0 before the source loop and read back after it:
// held in scalars instead, these values live across decodeBlock, where the scalar file is full (each one spills into a
// VGPR lane: 129 VGPRs in the counting form).
struct ReduceNormTile {
  uint64_t words;     // the tile's first accumulator word
  uint64_t sumSq;     // this (member, tile)'s slot of DecodeArgs::normPartials
  uint64_t nonFinite; // and of the counts behind them
  uint32_t numWords;  // words of this tile that the sources state
  uint32_t pad;
};
template <uint32_t FT, bool kRounded, uint32_t kThreads>
__device__ __forceinline__ void reduceNormTile(const ReduceNormTile* sTile, uint8_t* smem) {
  constexpr uint32_t kWaves = kThreads / 64u;
  reduceHandOver();  // the last source is in the accumulator; rings and LUT are free
  typedef __attribute__((address_space(1))) uint8_t* GlobalBytes;
  const ReduceNormTile t = *sTile;
  const uint32_t tileWords = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.numWords);
  const uint32_t* words = (const uint32_t*)(GlobalBytes)(uintptr_t)t.words;
  // (the thread's indices are derived here, like the source loop's own: nothing of this lives across decodeBlock)
  uint32_t tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  double sq = 0.0;
  uint32_t bad = 0;
  const uint32_t quads = tileWords / 4u;
#pragma unroll 4
  for (uint32_t q = tid; q < quads; q += kThreads) {
    const u32x4w v = ((const u32x4w4*)words)[q];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) normMeasure<FT, kRounded>(v[k], sq, bad);
  }
  if (tid < (tileWords & 3u)) normMeasure<FT, kRounded>(words[quads * 4u + tid], sq, bad);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    sq += __shfl_xor(sq, d, 64);
    bad += __shfl_xor(bad, d, 64);
  }
  double* sWaveSq = (double*)smem;
  uint32_t* sWaveCount = (uint32_t*)(sWaveSq + kWaves);
  if (lane == 0u) {
    sWaveSq[wave] = sq;
    sWaveCount[wave] = bad;
  }
  __syncthreads();
  if (tid == 0u) {
    double tileSq = sWaveSq[0];
    uint32_t tileBad = sWaveCount[0];
#pragma unroll
    for (uint32_t w = 1; w < kWaves; ++w) {
      tileSq += sWaveSq[w];
      tileBad += sWaveCount[w];
    }
    *(double*)(GlobalBytes)(uintptr_t)t.sumSq = tileSq;
    *(uint32_t*)(GlobalBytes)(uintptr_t)t.nonFinite = tileBad;
  }
}
constexpr uintptr_t kReduceRawTag = 1u;
__device__ __forceinline__ bool reduceIsRaw(const uint8_t* source) { return ((uintptr_t)source & kReduceRawTag) != 0u; }
typedef uint16_t u16n __attribute__((aligned(2)));
__device__ __forceinline__ uint32_t rawLoad16(const uint8_t* p) {
  return kNtEncLoads ? (uint32_t)__builtin_nontemporal_load((const u16n*)p) : (uint32_t)*(const u16n*)p;
}
__device__ __forceinline__ uint32_t rawLoad32(const uint8_t* p) {
  return kNtEncLoads ? __builtin_nontemporal_load((const uint32_t*)p) : *(const uint32_t*)p;
}
// a lane's 8 consecutive 16-bit words, two per dword: one 16-byte load, four 4-byte loads or eight 2-byte loads,
// whichever the row's base allows (align: 16, 4 or 2; block and group offsets are multiples of 16 bytes)
__device__ __forceinline__ u32x4w rawLoadGroup(const uint8_t* p, uint32_t align) {
  u32x4w w;
  if (align >= 16u) {
    w = kNtEncLoads ? __builtin_nontemporal_load((const u32x4w*)p) : *(const u32x4w*)p;
  } else if (align >= 4u) {
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) w[k] = rawLoad32(p + 4u * k);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) w[k] = rawLoad16(p + 4u * k) | (rawLoad16(p + 4u * k + 2u) << 16);
  }
  return w;
}
// This half's block of a raw source: n words of FT at src (0: the half has no block).  16-bit types: the whole 8-row
// groups in the wide layout (flushWords), four groups' loads in flight; what is left row by row (storeWord), as the
// tail path of decodeBlock leaves it.  float32: row by row, eight rows' loads in flight.
template <uint32_t FT, typename Sink>
__device__ __forceinline__ void reduceRawBlock(const Sink& sink, const uint8_t* src, uint32_t n, uint32_t hl, uint32_t align) {
  if constexpr (FT == kFloat32) {
    const uint32_t rows = n / 32u;
    uint32_t row = 0;
    for (; row + 8u <= rows; row += 8u) {
      typename Sink::Pre p[8];
      uint32_t w[8];
#pragma unroll
      for (uint32_t j = 0; j < 8u; ++j) {
        p[j] = sink.prefetchAcc(row + j);
        w[j] = rawLoad32(src + ((size_t)(row + j) * 32u + hl) * 4u);
      }
#pragma unroll
      for (uint32_t j = 0; j < 8u; ++j) sink.storeWord(row + j, w[j], p[j]);
    }
    for (; row * 32u + hl < n; ++row) {
      const typename Sink::Pre p = sink.prefetchAcc(row);
      sink.storeWord(row, rawLoad32(src + ((size_t)row * 32u + hl) * 4u), p);
    }
  } else {
    const uint32_t groups = n / (kGroupRows * 32u);
    uint32_t g = 0;
    for (; g + 4u <= groups; g += 4u) {
      typename Sink::GroupPre p[4];
      u32x4w w[4];
#pragma unroll
      for (uint32_t j = 0; j < 4u; ++j) {
        sink.prefetchGroupAcc(g + j, hl, p[j]);
        w[j] = rawLoadGroup(src + (g + j) * 512u + hl * 16u, align);
      }
#pragma unroll
      for (uint32_t j = 0; j < 4u; ++j) sink.flushWords(g + j, hl, w[j], p[j]);
    }
    for (; g < groups; ++g) {
      typename Sink::GroupPre p;
      sink.prefetchGroupAcc(g, hl, p);
      sink.flushWords(g, hl, rawLoadGroup(src + g * 512u + hl * 16u, align), p);
    }
    for (uint32_t row = groups * kGroupRows; row * 32u + hl < n; ++row) {
      const typename Sink::Pre p = sink.prefetchAcc(row);
      sink.storeWord(row, rawLoad16(src + (row * 32u + hl) * 2u), p);
    }
  }
}

// Between two sources of decodeReduceTile: source s - 1 is in the accumulator before source s asks for it (see there)
__device__ __forceinline__ void reduceHandOver() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// What a source's sink is told, for an archive and for a raw row alike: store or add, and (counting form) whether the
// sums are counted -- on the LAST source
__device__ __forceinline__ uint32_t reduceAccumulates(const DecodeArgs& a, uint32_t s) { return (s != 0u || a.accumulate != 0u) ? 1u : 0u; }
__device__ __forceinline__ bool reduceCounts(uint32_t s, uint32_t S) { return s + 1u == S; }
// (scaled forms that keep the factor in registers: it applies where the counting form counts)
template <typename Sink>
__device__ __forceinline__ void reduceScales(Sink& sink, const DecodeArgs& a, uint32_t s) {
  if constexpr (Sink::kScaled && !Sink::kStats) {
    sink.scale = a.scale;
    sink.scaleLast = reduceCounts(s, a.numSources) ? 1u : 0u;
    if constexpr (Sink::kUnit) sink.scaleLast = a.scale != 1.0f ? sink.scaleLast : 0u;
  }
}

// A raw source's turn in the source loop of decodeReduceTile: the hand-over barrier of an archive source, the sink set up
// as for one, and every half-wave's block through reduceRawBlock.  (Its lane indices are laundered like the loop's own.)
template <uint32_t FT, typename Sink>
__device__ __forceinline__ void reduceRawSource(const DecodeArgs& a, uint32_t b, const uint8_t* row, uint32_t s, uint32_t total, uint32_t tileFirst,
                                                uint32_t nb, uint32_t wave, uint32_t binsLds) {
  uint32_t tidS = threadIdx.x;
  asm volatile("" : "+v"(tidS));
  const uint32_t laneS = tidS & 63u;
  const uint32_t hl = laneS & 31u;
  const uint32_t block = tileFirst + wave * 2u + (laneS >= 32u ? 1u : 0u);
  const bool haveBlock = block < nb;
  if (s != 0u) reduceHandOver();
  Sink sink;
  sink.accumulate = reduceAccumulates(a, s);
  if constexpr (Sink::kStats) sink.bins = reduceCounts(s, a.numSources) ? binsLds + (laneS & (Sink::kStatSlots - 1u)) * 4u : 0u;
  reduceScales(sink, a, s);
  sink.init(a.out.ptr(b), row, total, (size_t)(haveBlock ? block : 0u) * kBlockSize, hl);
  const uint32_t left = haveBlock ? total - block * kBlockSize : 0u;
  const uint32_t align = ((uintptr_t)row & 15u) == 0u ? 16u : (((uintptr_t)row & 3u) == 0u ? 4u : 2u);
  reduceRawBlock<FT>(sink, row + (size_t)block * kBlockSize * decOutWordBytes(FT), left < kBlockSize ? left : kBlockSize, hl, align);
}

struct ReduceSource {  // verdict on one source (LDS)
  uint32_t ok;          // headers and pdf sum
  uint32_t total;       // words the ANS header states (ok)
  uint32_t totalWords;  // compressed words (ok)
  uint32_t report;      // what a decode of this source alone would write to outSize
};
constexpr uint32_t kMaxReduceSources = 64;

template <int P, uint32_t FT, uint32_t kTileBlocks, bool kStats = false, bool kMixed = false, bool kScaled = false, bool kNorm = false>
__device__ __forceinline__ void decodeReduceTile(const DecodeArgs& a) {
  static_assert(FT != 0u, "decode-reduce: float archives only");
  static_assert(!kNorm || (kMixed && kScaled), "the norm forms are forms of the scaled mixed kernels");
  constexpr uint32_t kSlots = kStats ? decStatsSlots(kTileBlocks) : 0u;
  using Sink = AccumSink<FT, kSlots, kScaled, kNorm>;
  constexpr uint32_t kDecThreads = decThreads(kTileBlocks), kWaves = kDecThreads / 64u;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint2* sLut = (uint2*)(smem + kTileBlocks * kRingBytes);
  constexpr uint32_t kXpose = decXposeBytes(P, FT, kTileBlocks);
  // the verdicts live in the ring area behind the LUT-build scratch (2 KiB + a few words at offset 0), which source 0
  // fills while slower waves may still be reading them
  static_assert(kTileBlocks * kRingBytes >= 4096u + kMaxReduceSources * sizeof(ReduceSource) + 4u * kWaves, "");
  ReduceSource* sSrc = (ReduceSource*)(smem + 4096u);
  uint32_t* sWaveBad = (uint32_t*)(sSrc + kMaxReduceSources);

  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  uint32_t b, tile;
  if (!decodeTileOf(a, blockIdx.x, &b, &tile)) return;  // uniform
  const uint32_t S = a.numSources, first = b * S;
  const uint32_t capacity = a.out.size(b);
  const uint32_t tileFirst = tile * kTileBlocks;
  // (a rectangle is laid out for the largest capacity: no valid member has blocks past its own)
  if (tile != 0 && (uint64_t)tileFirst * kBlockSize >= capacity) return;  // uniform
  // kStats: the bins lie behind rings, LUT and store buffers; they are zero after the first barrier below
  constexpr uint32_t kBinsAt = kTileBlocks * kRingBytes + decLutBytes(P, kTileBlocks) + kTileBlocks * kXpose;
  constexpr uint32_t kNormTileAt = kBinsAt + (kStats ? decStatsBinBytes(kTileBlocks) + kSlots * 4u : 0u);  // kNorm: ReduceNormTile
  if constexpr (kStats) {
    for (uint32_t i = tid; i < kNumSymbols * kSlots / 4u; i += kDecThreads) ((uint4*)(smem + kBinsAt))[i] = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (kScaled) {  // the factor, one per slot column behind the bins (AccumSink::factor)
      if (tid < kSlots) ((float*)(smem + kBinsAt + decStatsBinBytes(kTileBlocks)))[tid] = a.scale;
    }
  }

  // ---- 1. validate every source ----
  for (uint32_t s = wave; s < S; s += kWaves) {  // (everything here is wave-uniform)
    const uint8_t* archive = a.in.ptr(first + s);
    const uint64_t inBytes = a.inBytes[first + s];
    ReduceSource r = {0u, 0u, 0u, 0u};
    bool raw = false;
    if constexpr (kMixed) raw = reduceIsRaw(archive);
    if (raw) {  // the row states its count as a header would
      const uint32_t words = (uint32_t)(inBytes / decOutWordBytes(FT));
      r.ok = (kStats ? words == capacity : words <= capacity) ? 1u : 0u;
      r.total = r.report = words;
    } else if (inBytes >= sizeof(FloatHeader)) {
      const FloatHeader fh = *(const FloatHeader*)archive;
      r.report = fh.size;
      const bool fhOk = fh.magicAndVersion == ((kFloatMagic << 16) | kFloatVersion) && (fh.options & 0xfu) == FT && fh.size <= capacity &&
          (uint64_t)sizeof(FloatHeader) + floatUncompDataSize(FT, fh.size) + sizeof(AnsHeader) <= inBytes;
      if (fhOk) {
        const uint8_t* ans = archive + ansOffsetInArchive(FT, fh.size);
        const AnsHeader header = *(const AnsHeader*)ans;
        const uint32_t nb = header.numBlocks, total = header.totalUncompressedWords;
        bool ok = capacity >= total && header.magicAndVersion == ((kAnsMagic << 16) | kAnsVersion) && (header.options & 0xfu) == (uint32_t)P &&
            fh.size == total && nb == divUp(total, kBlockSize) &&
            (uint64_t)ansOffsetInArchive(FT, total) + ansOverhead(nb) + 2ull * header.totalCompressedWords <= inBytes;
        if constexpr (kStats) ok = ok && total == capacity;  // the words the encoder codes are the words that are counted
        if (ok && nb != 0u) {
          // the probabilities of a non-empty element sum to 2^P: four per lane, then over the wave
          const uint2 raw = *(const uint2*)(ans + sizeof(AnsHeader) + 8u * lane);
          uint32_t sum = (raw.x & 0xffffu) + (raw.x >> 16) + (raw.y & 0xffffu) + (raw.y >> 16);
#pragma unroll
          for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
          ok = sum == (1u << P);
        }
        r.ok = ok ? 1u : 0u;
        r.total = total;
        r.totalWords = header.totalCompressedWords;
        r.report = total;
      }
    }
    if (lane == 0u) sSrc[s] = r;
  }
  __syncthreads();
  const uint32_t total = sSrc[0].total, report = sSrc[0].report;
  bool memberOk = true;
  for (uint32_t s = 0; s < S; ++s) memberOk = memberOk && sSrc[s].ok != 0u && sSrc[s].total == total;
  if (!memberOk) {  // uniform, and the same in every tile of the member: nothing of it is stored
    if (tile == 0 && tid == 0) {
      if (a.outSuccess) a.outSuccess[b] = 0;
      if (a.outSize) a.outSize[b] = report;
    }
    return;
  }
  const uint32_t nb = divUp(total, kBlockSize);
  if (tileFirst >= nb && tile != 0) return;  // uniform
  const uint32_t ansOff = ansOffsetInArchive(FT, total);
  if constexpr (kNorm) {  // for reduceNormTile, behind everything else in LDS (visible after any of the barriers below)
    if (tid == 0u) {
      ReduceNormTile t;
      t.words = (uint64_t)(uintptr_t)((const uint32_t*)a.out.ptr(b) + (size_t)tileFirst * kBlockSize);
      const size_t slots = (size_t)a.numInBatch * a.maxTiles, at = (size_t)b * a.maxTiles + tile;
      t.sumSq = (uint64_t)(uintptr_t)(a.normPartials + at);
      t.nonFinite = (uint64_t)(uintptr_t)((uint32_t*)(a.normPartials + slots) + at);
      t.numWords = total - tileFirst * kBlockSize < kTileBlocks * kBlockSize ? total - tileFirst * kBlockSize : kTileBlocks * kBlockSize;
      t.pad = 0u;
      *(ReduceNormTile*)(smem + kNormTileAt) = t;
    }
  }
  {
    // block i of source s must be what an encoder can produce (decodeTile's blockOk)
    bool allBlocksOk = true;
    for (uint32_t i = tid; i < S * nb; i += kDecThreads) {
      const uint32_t s = i / nb, blk = i - s * nb;
      if constexpr (kMixed) {
        if (reduceIsRaw(a.in.ptr(first + s))) continue;  // a raw row has no descriptors
      }
      const uint2 bw = ((const uint2*)(a.in.ptr(first + s) + ansOff + ansBlockWordsOffset(nb)))[blk];
      const uint32_t want = (blk + 1u < nb) ? kBlockSize : total - blk * kBlockSize;
      const bool ok = (bw.x >> 16) == want && (bw.y & (kBlockAlignWords - 1u)) == 0u &&
          (uint64_t)bw.y + roundUp(bw.x & 0xffffu, kBlockAlignWords) <= (uint64_t)sSrc[s].totalWords;
      allBlocksOk = allBlocksOk & ok;
    }
    const bool waveBad = __ballot(!allBlocksOk) != 0ull;
    if (lane == 0u) sWaveBad[wave] = waveBad ? 1u : 0u;
  }
  __syncthreads();
  uint32_t anyBad = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) anyBad |= sWaveBad[w];
  if (tile == 0 && tid == 0) {
    if (a.outSuccess) a.outSuccess[b] = anyBad ? 0 : 1;
    if (a.outSize) a.outSize[b] = report;
  }
  if (anyBad != 0u || tileFirst >= nb) return;  // uniform

  // ---- 2. one source after the other ----
  const uint32_t ldsBase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem;
  constexpr bool kCompact = decCompactLut(P, kTileBlocks);
  const bool wide = kXpose != 0u;  // (accumulators are float-aligned, the host checks it)
  uint32_t* sCdf = (uint32_t*)smem;
  uint32_t* sPdf = sCdf + kNumSymbols;

#pragma unroll 1
  for (uint32_t s = 0; s < S; ++s) {
    // Everything a lane derives from its index is derived HERE, from a value the compiler cannot see through: hoisted
    // out of the loop, these addresses and offsets stay in registers across decodeBlock (151 VGPRs: one wave per SIMD,
    // i.e. one of two workgroups per CU, fewer than k_ans_decode_accum; recomputed per source they cost a few dozen VALU
    // per source).  tests/test_reduce_kernel_resources.py holds the 16-bit forms to the 128 VGPRs of four waves per SIMD.
    if constexpr (kMixed) {
      const uint8_t* src = a.in.ptr(first + s);
      if (reduceIsRaw(src)) {  // uniform.  A raw row: no LUT, no ring, no row loop
        reduceRawSource<FT, Sink>(a, b, src - kReduceRawTag, s, total, tileFirst, nb, wave, ldsBase + kBinsAt);
        continue;
      }
    }
    uint32_t tidS = threadIdx.x;
    asm volatile("" : "+v"(tidS));
    const uint32_t laneS = tidS & 63u;
    const bool upper = laneS >= 32u;
    const uint32_t hl = laneS & 31u;
    const uint32_t hw = wave * 2u + (upper ? 1u : 0u);
    const uint32_t block = tileFirst + hw;
    const bool haveBlock = block < nb;
    // (a half without a block points at its wave's first block: its prefetches stay inside archive and accumulator)
    const uint32_t sinkBlock = haveBlock ? block : (block & ~1u);
    const uint32_t xpose = ldsBase + kTileBlocks * kRingBytes + decLutBytes(P, kTileBlocks) + hw * kXpose;
    const uint32_t ringLds = ldsBase + hw * kRingBytes;
    const uint8_t* archive = a.in.ptr(first + s);
    const uint8_t* ans = archive + ansOff;
    uint2 pdfRaw = make_uint2(0u, 0u), bwMine = make_uint2(0u, 0u);
    uint32_t state = 0;
    if (wave == 0) pdfRaw = ((const uint2*)(ans + sizeof(AnsHeader)))[laneS];  // pdf[4 lane .. 4 lane + 3]
    if (haveBlock) {
      bwMine = ((const uint2*)(ans + ansBlockWordsOffset(nb)))[block];
      state = ((const uint32_t*)(ans + ansStatesOffset()))[block * 32u + hl];
    }
    if (s != 0u) reduceHandOver();  // (the barrier also frees LUT and rings)
    const uint32_t n = bwMine.x >> 16, numWords = bwMine.x & 0xffffu;
    const uint8_t* gwords = ans + ansOverhead(nb) + 2u * (size_t)bwMine.y;
    Sink sink;
    sink.accumulate = reduceAccumulates(a, s);
    if constexpr (kStats) sink.bins = reduceCounts(s, S) ? ldsBase + kBinsAt + (laneS & (kSlots - 1u)) * 4u : 0u;
    reduceScales(sink, a, s);
    sink.init(a.out.ptr(b), archive, total, (size_t)sinkBlock * kBlockSize, hl);
    // uniform per wave (the staging mode is this source's own; full / tail follow the word count, the same for all)
    const uint32_t nFirst = __shfl(n, 0, 64);
    const uint32_t nSecond = __shfl(n, 32, 64);
    const uint32_t wFirst = __shfl(numWords, 0, 64);
    const uint32_t wSecond = __shfl(numWords, 32, 64);
    const bool noRing = wFirst <= kRingBytes / 2u && wSecond <= kRingBytes / 2u;
    const bool fullPair = nFirst == kBlockSize && nSecond == kBlockSize;
    const bool fullSingle = nFirst == kBlockSize && nSecond == 0u;
    DecodePreOf<typename Sink::GroupPre> pre;
    if ((fullPair || fullSingle) && noRing) decodePrefetch<FT>(pre, gwords, numWords, sink, hl, wide);

    // the LUT of this source (see decodeTile): wave 0 scans the 256 pdfs, every thread fills its slots
    if (wave == 0) {
      const uint32_t p0 = pdfRaw.x & 0xffffu, p1 = pdfRaw.x >> 16, p2 = pdfRaw.y & 0xffffu, p3 = pdfRaw.y >> 16;
      const uint32_t mine = p0 + p1 + p2 + p3;
      const uint32_t base = waveInclusiveScan(mine, laneS) - mine;
      ((uint4*)sCdf)[laneS] = make_uint4(base, base + p0, base + p0 + p1, base + p0 + p1 + p2);
      ((uint4*)sPdf)[laneS] = make_uint4(p0, p1, p2, p3);
    }
    __syncthreads();
    for (uint32_t x = tidS; x < (1u << P); x += kDecThreads) {
      uint32_t lo = 0, hi = kNumSymbols;  // the last symbol with cdf <= x
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const uint32_t mid = (lo + hi) >> 1;
        const bool le = sCdf[mid] <= x;
        lo = le ? mid : lo;
        hi = le ? hi : mid;
      }
      if (kCompact) ((uint32_t*)sLut)[x] = (sPdf[lo] & 0xfffu) | (((x - sCdf[lo]) & 0xfffu) << 12) | (lo << 24);
      else sLut[x] = make_uint2((sPdf[lo] & 0xfffu) | (lo << 24), (x - sCdf[lo]) & 0xfffu);
    }
    __syncthreads();  // LUT visible, scratch free

    // the dispatch of decodeTile
#define DGPU_REDUCE_FULL(WIDE, IDLE, NORING) \
  decodeBlock<P, FT, true, WIDE, IDLE, kCompact, NORING, NORING, false, Sink>(xpose, state, n, kRowsPerBlock / kGroupRows, gwords, numWords, ringLds, sLut, sink, hl, upper, &pre)
#define DGPU_REDUCE_TAIL(WIDE, IDLE, NORING) \
  decodeBlock<P, FT, true, WIDE, IDLE, kCompact, NORING, false, true, Sink>(xpose, state, n, groups, gwords, numWords, ringLds, sLut, sink, hl, upper, nullptr, topRows)
    if (fullPair) {
      if (wide) {
        if (noRing) DGPU_REDUCE_FULL(true, false, true); else DGPU_REDUCE_FULL(true, false, false);
      } else {
        if (noRing) DGPU_REDUCE_FULL(false, false, true); else DGPU_REDUCE_FULL(false, false, false);
      }
    } else if (fullSingle) {
      if (wide) {
        if (noRing) DGPU_REDUCE_FULL(true, true, true); else DGPU_REDUCE_FULL(true, true, false);
      } else {
        if (noRing) DGPU_REDUCE_FULL(false, true, true); else DGPU_REDUCE_FULL(false, true, false);
      }
    } else {
      const uint32_t maxN = nFirst > nSecond ? nFirst : nSecond;
      const uint32_t maxRows = divUp(maxN, 32u);
      const uint32_t fullRows = (nSecond ? nSecond : nFirst) / 32u;  // (the last block of the wave is the partial one)
      const uint32_t groups = fullRows / kGroupRows;
      const uint32_t topRows = maxRows - groups * kGroupRows;
      const bool tailPair = nFirst == kBlockSize && nSecond != 0u, tailSingle = nFirst != 0u && nSecond == 0u;
      if (tailPair && groups != 0u) {
        if (wide) {
          if (noRing) DGPU_REDUCE_TAIL(true, false, true); else DGPU_REDUCE_TAIL(true, false, false);
        } else {
          if (noRing) DGPU_REDUCE_TAIL(false, false, true); else DGPU_REDUCE_TAIL(false, false, false);
        }
      } else if (tailSingle && groups != 0u) {
        if (wide) {
          if (noRing) DGPU_REDUCE_TAIL(true, true, true); else DGPU_REDUCE_TAIL(true, true, false);
        } else {
          if (noRing) DGPU_REDUCE_TAIL(false, true, true); else DGPU_REDUCE_TAIL(false, true, false);
        }
      } else {
        decodeBlock<P, FT, false, false, false, kCompact, false, false, false, Sink>(xpose, state, n, divUp(maxRows, kGroupRows), gwords, numWords, ringLds, sLut, sink, hl, upper);
      }
    }
#undef DGPU_REDUCE_FULL
#undef DGPU_REDUCE_TAIL
  }
  if constexpr (kStats) {
    // the tile's counts join the member's: bin-major, so a bin's slots are consecutive (histFold)
    __syncthreads();
    const uint32_t* bins = (const uint32_t*)(smem + kBinsAt);
    for (uint32_t c = tid; c < kNumSymbols; c += kDecThreads) {
      uint32_t sum = 0;
#pragma unroll
      for (uint32_t k = 0; k < kSlots / 4u; ++k) {
        const uint4 v = ((const uint4*)(bins + c * kSlots))[k];
        sum += v.x + v.y + v.z + v.w;
      }
      if (sum) __hip_atomic_fetch_add(a.stats + (size_t)b * kNumSymbols + c, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if constexpr (kNorm) reduceNormTile<FT, kStats, kDecThreads>((const ReduceNormTile*)(smem + kNormTileAt), smem);
}

// grid = the (element, tile) pairs in the order of DecodeArgs::order
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode(DecodeArgs a) {
  decodeTile<P, FT, kTileBlocks, DecodeForm::kWhole>(a);
}

// Ranged form: grid = the listed tiles of the ranges (kDecOrderMap; DecodeArgs::firstBlock / numBlocks / inBytes set).
// Built for 16- and 4-block tiles.
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_range(DecodeArgs a) {
  decodeTile<P, FT, kTileBlocks, DecodeForm::kRanged>(a);
}

// Accumulating form: grid and order as k_ans_decode; DecodeArgs::out holds float32 accumulators, DecodeArgs::accumulate
// says whether they are added to or overwritten.  Built for the float types, 16- and 4-block tiles.
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_accum(DecodeArgs a) {
  decodeTile<P, FT, kTileBlocks, DecodeForm::kAccum>(a);
}

// Scaled form: grid, order and LDS as k_ans_decode; every word leaves multiplied by the member's factor
// (DecodeArgs::scalePtr / scaleStride / scale).  Built for the float types, 16- and 4-block tiles.
__host__ __device__ constexpr uint32_t decScaledLdsBytes(int P, uint32_t ft, uint32_t tileBlocks) { return decLdsBytes(P, ft, tileBlocks); }
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_scaled(DecodeArgs a) {
  static_assert(FT != 0u, "scaled decode: float archives only");
  decodeTile<P, FT, kTileBlocks, DecodeForm::kWholeScaled>(a);
}

// Scaled accumulating form: k_ans_decode_accum with the widened word multiplied by the member's factor before the store
// or the add (DecodeArgs::scalePtr / scaleStride / scale).  Grid, order and LDS as k_ans_decode_accum.
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_accum_scaled(DecodeArgs a) {
  static_assert(FT != 0u, "accumulating decode: float archives only");
  decodeTile<P, FT, kTileBlocks, DecodeForm::kAccumScaled>(a);
}

// Updating form: k_ans_decode_accum_scaled whose outputs are 16-bit tensors of the archive's type, rounded stochastically
// (DecodeArgs::seedPtr / seed / firstMember).  Grid, order and LDS as k_ans_decode_accum.  float16 and bfloat16 only.
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_update(DecodeArgs a) {
  static_assert(FT == kFloat16 || FT == kBFloat16, "decode-update: 16-bit float archives only");
  decodeTile<P, FT, kTileBlocks, DecodeForm::kUpdate>(a);
}

// Reducing form: grid and order as k_ans_decode_accum, DecodeArgs::numSources archives per accumulator (decodeReduceTile).
// Built for the float types, 16- and 4-block tiles.
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_reduce(DecodeArgs a) {
  decodeReduceTile<P, FT, kTileBlocks>(a);
}

// Counting form (reduce-compress): k_ans_decode_reduce that also leaves, in DecodeArgs::stats, the exponent histogram of
// the sums rounded to FT (decodeReduceTile, kStats).  Built for float16 / bfloat16, 16- and 4-block tiles.
__host__ __device__ constexpr uint32_t decReduceStatsLdsBytes(int P, uint32_t ft, uint32_t tileBlocks) {
  return decLdsBytes(P, ft, tileBlocks) + decStatsBinBytes(tileBlocks);
}
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_reduce_stats(DecodeArgs a) {
  static_assert(FT == kFloat16 || FT == kBFloat16, "the archive types of a cast");
  decodeReduceTile<P, FT, kTileBlocks, true>(a);
}

// Mixed forms: k_ans_decode_reduce and k_ans_decode_reduce_stats whose sources are archives or raw rows of FT words
// (DecodeArgs::sourceKind; decodeReduceTile, kMixed).  Built for the types and tile sizes of their plain siblings.
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_reduce_mixed(DecodeArgs a) {
  decodeReduceTile<P, FT, kTileBlocks, false, true>(a);
}
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_reduce_mixed_stats(DecodeArgs a) {
  static_assert(FT == kFloat16 || FT == kBFloat16, "the archive types of a cast");
  decodeReduceTile<P, FT, kTileBlocks, true, true>(a);
}

// Scaled forms of the two mixed kernels: the last source's store leaves fl32(sum * DecodeArgs::scale), and the counting
// form counts it (decodeReduceTile, kScaled).  The counting form keeps the factor in LDS behind its bins.
__host__ __device__ constexpr uint32_t decReduceStatsScaledLdsBytes(int P, uint32_t ft, uint32_t tileBlocks) {
  return decReduceStatsLdsBytes(P, ft, tileBlocks) + decStatsSlots(tileBlocks) * 4u;
}
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_reduce_mixed_scaled(DecodeArgs a) {
  decodeReduceTile<P, FT, kTileBlocks, false, true, true>(a);
}
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_reduce_mixed_stats_scaled(DecodeArgs a) {
  static_assert(FT == kFloat16 || FT == kBFloat16, "the archive types of a cast");
  decodeReduceTile<P, FT, kTileBlocks, true, true, true>(a);
}

// Norm forms of the two scaled kernels: when a tile's last source is stored, the workgroup also measures what it left --
// the squared norm of the finite words and the count of the others, per (member, tile), in DecodeArgs::normPartials
// (decodeReduceTile, kNorm).  They take a factor of 1 too, and then multiply nothing.  LDS: the scaled forms' and a ReduceNormTile.
__host__ __device__ constexpr uint32_t decReduceNormLdsBytes(int P, uint32_t ft, uint32_t tileBlocks, bool stats) {
  return (stats ? decReduceStatsScaledLdsBytes(P, ft, tileBlocks) : decLdsBytes(P, ft, tileBlocks)) + (uint32_t)sizeof(ReduceNormTile);
}
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_reduce_mixed_norm(DecodeArgs a) {
  decodeReduceTile<P, FT, kTileBlocks, false, true, true, true>(a);
}
template <int P, uint32_t FT, uint32_t kTileBlocks>
__global__ __launch_bounds__(decThreads(kTileBlocks)) void k_ans_decode_reduce_mixed_stats_norm(DecodeArgs a) {
  static_assert(FT == kFloat16 || FT == kBFloat16, "the archive types of a cast");
  decodeReduceTile<P, FT, kTileBlocks, true, true, true, true>(a);
}

// One wavefront per member adds the member's tile partials: lane l those of tiles l, l + 64, ... in tile order, then the
// fixed tree over the lanes.  A member that failed, or is empty, stored no partial: its slots hold the zeros they were
// launched with, and so do its results.  Either output may be absent.
struct ReduceNormFinishArgs {
  const double* partials;  // DecodeArgs::normPartials
  uint32_t numInBatch, maxTiles;
  double* outSumSq;        // [numInBatch] nullable
  uint32_t* outNonFinite;  // [numInBatch] nullable
};
constexpr uint32_t kNormFinishThreads = 256;
__host__ __device__ constexpr size_t reduceNormPartialBytes(size_t numInBatch, size_t maxTiles) { return numInBatch * maxTiles * 12u; }
__global__ __launch_bounds__(kNormFinishThreads) void k_reduce_norm_finish(ReduceNormFinishArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = blockIdx.x * (kNormFinishThreads / 64u) + (threadIdx.x >> 6);
  if (b >= a.numInBatch) return;  // wave-uniform
  const double* partSq = a.partials + (size_t)b * a.maxTiles;
  const uint32_t* partBad = (const uint32_t*)(a.partials + (size_t)a.numInBatch * a.maxTiles) + (size_t)b * a.maxTiles;
  double sq = 0.0;
  uint32_t bad = 0;
  for (uint32_t t = lane; t < a.maxTiles; t += 64u) {
    sq += partSq[t];
    bad += partBad[t];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    sq += __shfl_xor(sq, d, 64);
    bad += __shfl_xor(bad, d, 64);
  }
  if (lane == 0u) {
    if (a.outSumSq) a.outSumSq[b] = sq;
    if (a.outNonFinite) a.outNonFinite[b] = bad;
  }
}

}  // namespace dgpu
