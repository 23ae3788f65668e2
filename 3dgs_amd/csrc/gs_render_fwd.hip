// gs_render_fwd.hip -- per-tile alpha compositing, forward, for gfx950 (the backward: gs_render_bwd.hip).
//
// Semantics: render_image of the reference (cuda/render.cu:6-135) -- front-to-back blending of each 16x16 tile's depth-
// sorted list with the 1/255 alpha floor, the 0.99 cap and the T < 1e-4 stop.
//
// Design (not the reference's one-warp-per-tile, 8-pixels-per-lane layout), shared with the backward:
//   * one 256-thread workgroup per tile = four wave64s; every 16-lane ROW of a wave owns one 4x4 pixel block,
//     one pixel per lane;
//   * the tile's list is consumed in batches (256 entries forward, 128 backward): every thread gathers ONE gaussian
//     (three 16-byte loads of a 48-byte record, or the reference's four arrays), works out which of the tile's 16
//     blocks the ellipse alpha >= 1/255 can reach (gs::block_hits; the forward hands these masks to the backward),
//     and parks the record in LDS in the form the loops evaluate (gs::stage_record);
//   * each wave compacts, per row, the batch's slots that hit the row's block into a byte list in LDS, and every
//     row walks ITS OWN list: in one loop trip the four rows of a wave work on four different (gaussian, block)
//     pairs and a wave's trip count is the longest of its four lists -- on the benchmark scene 1.65x fewer trips
//     than visiting (gaussian, 8x8 quadrant) pairs (tests/analysis/model_trips.py).  Skipping is exact: a skipped
//     gaussian has alpha < 1/255 on every pixel of the block;
//   * forward: two list entries per trip; a row whose 16 pixels are saturated gets no list, a wave stops when its 64
//     pixels are saturated, the workgroup when all four waves have; on the side it clears the gradient rows the
//     backward accumulates into (the kernel leaves most of the HBM bandwidth unused).  33 VALU per two-entry trip (r04:
//     the 0.99 cap lives in the exponent's clamp, a pixel's T is zeroed only in the trip that saturates it).
// The two tables of the forward's long lists (fwd_segments_table_kernel in front of it, fwd_segments_combine_kernel
// behind it) live here too.
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_render.h"

#if GS_STAMP
__device__ unsigned long long gs_stamp_fwd[(1 << 16) * GS_STAMP_WORDS];  // render_bwd's layout (gs_render_bwd.hip), phases mapped below
#endif

namespace gs {

// ---- r05: long lists in segments, forward (gs_render.h: FwdSegments) ------------------------------------------------
typedef __attribute__((address_space(1))) unsigned long long gs_gu64;
__device__ __forceinline__ void granule_store(unsigned long long *g, unsigned int epoch, float v) {
  __hip_atomic_store((gs_gu64 *)g, ((unsigned long long)epoch << 32) | __float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool granule_load(const unsigned long long *g, unsigned int epoch, float &v) {
  const unsigned long long x = __hip_atomic_load((gs_gu64 *)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  v = __uint_as_float((unsigned int)x);
  return (unsigned int)(x >> 32) == epoch;
}
// T in front of segment k's first entry from what the blocks in front have published: the nearest block q < k whose
// final T is out (F_q = P_(q+1)) and the products t_(q+1) .. t_(k-1) of the blocks behind it, multiplied up from the left
// -- whichever q a thread finds, the value is the same left fold.  false: the poll budget ran out.
// (segment j of the tile lives in storage slot base[j] + rank: t at gran[slot], F at gran[cap + slot])
__device__ __forceinline__ bool resolve_prefix(const FwdSegments &fs, int rank, int tid, int k, int budget, float &prefix) {
  const unsigned long long *gt = fs.granules + (size_t)rank * 256 + tid, *gf = gt + (size_t)fs.cap * 256;
  for (int polls = 0;;) {
    int q = -1;
    float v = 0.0f;
    for (int j = k - 1; j >= 0; --j) {
      const size_t at = (size_t)fs.base[j] * 256;
      if (granule_load(gf + at, fs.epoch, v)) { q = j; break; }
      float t;
      if (!granule_load(gt + at, fs.epoch, t)) break;
    }
    if (q >= 0) {
      for (int j = q + 1; j < k; ++j) {
        float t;
        (void)granule_load(gt + (size_t)fs.base[j] * 256, fs.epoch, t);  // (seen on the way down: published values stay)
        v = v * t;
      }
      prefix = v;
      return true;
    }
    if (++polls >= budget) return false;
    __builtin_amdgcn_s_sleep(32);
  }
}

// the forward loop's read of the record's second array: (c2, log2 opa), and in depth mode z from the slot behind them
template <bool kDepth>
__device__ __forceinline__ void fwd_r1(const char *r1b, int off, float2 &b, float &z) {
  if constexpr (kDepth) {
    const float4 q = *reinterpret_cast<const float4 *>(r1b + off);
    b = make_float2(q.x, q.y);
    z = q.z;
  } else {
    b = *reinterpret_cast<const float2 *>(r1b + off);
  }
}

// Phase A: the product of (1 - alpha) over the entries [begin, end) of the tile's list, per pixel -- the forward's loop
// without colour, stop test and saturation bookkeeping, the same alpha values in the same order, so that the running
// product is bit for bit the one phase C multiplies up.  `fold`: the product segment by segment from the left,
// ((t_0 t_1) t_2) ..., the order in which collect_prefix takes the published values.
template <bool kPacked>
__device__ __forceinline__ float fwd_t_product(const float4 *__restrict__ recs, const RawSplats &raw,
                                               const int *__restrict__ sorted, int start, int begin, int end, bool fold,
                                               float tx0, float ty0, float fpx, float fpy, int tid, float4 *s_r0,
                                               float4 *s_r1, float4 *s_r2, unsigned short *s_list) {
  const char *r0b = reinterpret_cast<const char *>(s_r0), *r1b = reinterpret_cast<const char *>(s_r1);
  const char *r2b = reinterpret_cast<const char *>(s_r2);
  float tl = 1.0f, pref = 1.0f;
  for (int base = begin; base < end; base += kBatch) {
    const int count = min(kBatch, end - base);
    int t = tid;
    asm volatile("" : "+v"(t));
    if (fold && base > begin && base % kSegEntries == 0) { pref = pref * tl; tl = 1.0f; }
    __syncthreads();
    if (t < count) {
      const int g = sorted[start + base + t];
      SplatRec s = load_record<kPacked>(g, recs, raw);
      const unsigned int hits = block_hits(s, tx0, ty0);
      stage_record(s);
      s.r1.w = __uint_as_float(hits);
      s.r2.w = s.r1.y > kLog2AlphaMax ? kLog2AlphaMax : s.r1.y;
      s_r0[t] = s.r0; s_r1[t] = s.r1; s_r2[t] = s.r2;
    }
    __syncthreads();
    unsigned short *lists = s_list + (t >> 6) * 4 * kListStride;
    const unsigned int list_lds =
        (unsigned int)(size_t)(__attribute__((address_space(3))) const unsigned short *)(lists + ((t >> 4) & 3) * kListStride);
    const RowCounts rc = build_row_lists<kListStride>(s_r1, lists, count, t >> 6, t & 63, kBatch, kBatch, kBatch, kBatch, 2);
    const int trips = max(max(rc.c0, rc.c1), max(rc.c2, rc.c3));
    for (int i = 0; i < trips; i += 2) {
      int off0, off1;
      asm volatile("ds_read_u16 %0, %2\n\tds_read_u16 %1, %2 offset:2\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(off0), "=&v"(off1) : "v"(list_lds + 2 * i) : "memory");
      const float4 a0 = *reinterpret_cast<const float4 *>(r0b + off0), a1 = *reinterpret_cast<const float4 *>(r0b + off1);
      const float2 b0 = *reinterpret_cast<const float2 *>(r1b + off0), b1 = *reinterpret_cast<const float2 *>(r1b + off1);
      const float l0 = *reinterpret_cast<const float *>(r2b + off0 + 12), l1 = *reinterpret_cast<const float *>(r2b + off1 + 12);
      float al0 = staged_alpha_capped(a0.z, a0.w, b0.x, b0.y, l0, a0.x - fpx, a0.y - fpy);
      float al1 = staged_alpha_capped(a1.z, a1.w, b1.x, b1.y, l1, a1.x - fpx, a1.y - fpy);
      al0 = al0 > kAlphaMin ? al0 : 0.0f;
      al1 = al1 > kAlphaMin ? al1 : 0.0f;
      asm volatile("" : "+v"(al0), "+v"(al1));
      tl = __builtin_fmaf(-al0, tl, tl);
      tl = __builtin_fmaf(-al1, tl, tl);
    }
  }
  return fold ? pref * tl : tl;
}

// One segment of a long list (gs_render.h: FwdSegments).
template <bool kPacked, bool kDepth, bool kInv = false, bool kMom = false>
__device__ __forceinline__ void fwd_segment_block(const float4 *__restrict__ recs, const RawSplats &raw,
                                                  const int *__restrict__ sorted, const int *__restrict__ ranges,
                                                  int width, int height, int ntx, unsigned short *__restrict__ masks_out,
                                                  const FwdSegments &fs, int blk, float4 *s_r0, float4 *s_r1,
                                                  float4 *s_r2, unsigned short *s_list, const DepthMaps &dm) {
  const int2 bk = fs.blocks[blk];
  const int tile = bk.x, k = bk.y & 0xFFFF;
  const bool side_by_side = (bk.y >> 30) != 0;  // a thin layer (fwd_segments_table_kernel)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, row = lane >> 4, j = lane & 15;
  if (tid == 0) {
    s_r0[kBatch] = s_r2[kBatch] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s_r1[kBatch] = sentinel_r1();
  }
  const int tile_x = tile % ntx, tile_y = tile / ntx;
  const int px = tile_x * 16 + (wave & 1) * 8 + (row & 1) * 4 + (j & 3);
  const int py = tile_y * 16 + (wave >> 1) * 8 + (row >> 1) * 4 + (j >> 2);
  const bool inside = px < width && py < height;
  const float fpx = (float)px, fpy = (float)py;
  const float tx0 = (float)(tile_x * 16), ty0 = (float)(tile_y * 16);
  const int start = ranges[tile], total = ranges[tile + 1] - start;
  const int m = (total + kSegEntries - 1) / kSegEntries;
  const int a = k * kSegEntries, b = min(total, a + kSegEntries);
  // this block's storage slot is its index; the slot of the segment in front: base[k - 1] + the tile's rank
  const int rank = fs.rank[tile];
  unsigned long long *gran_t = fs.granules + (size_t)blk * 256 + tid, *gran_f = gran_t + (size_t)fs.cap * 256;
  float4 *part = fs.part + (size_t)blk * 256 + tid;
  int *stop = fs.stop + (size_t)blk * 256 + tid;

  float prefix = 1.0f;
  if (k > 0) {
    // Is the block in front done already?  (The blocks are dispatched layer by layer -- all segments 0, then all segments
    // 1, ...: where a layer fills the chip, the layer behind it starts when it is through.)  Then T is simply what it left
    // behind, nobody behind this block can be waiting for its product yet either, so phase A is skipped: its final T will
    // do.  And if no pixel of the tile is left, neither has this segment anything to add.
    float f = 0.0f;
    const bool have = granule_load(fs.granules + ((size_t)fs.cap + fs.base[k - 1] + rank) * 256 + tid, fs.epoch, f);
    const bool all_have = __syncthreads_and(have ? 1 : 0);
    if (all_have) {
      prefix = f;
      if (__syncthreads_and(!inside || f < kTMin ? 1 : 0)) {
        if (k < m - 1) granule_store(gran_f, fs.epoch, 0.0f);
        *part = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if constexpr (kDepth) dm.part[(size_t)blk * 256 + tid] = 0.0f;
        if constexpr (kMom) dm.part2[(size_t)blk * 256 + tid] = 0.0f;
        *stop = -2;
        return;
      }
    } else {
      // In a thin layer the segments of a list run side by side: the blocks behind need this segment's product before
      // its compositing.  In a thick one the block in front is about to finish (it was dispatched a layer earlier) and the
      // other blocks of this CU keep its SIMDs busy meanwhile: waiting costs less than the product pass.
      if (side_by_side && k < m - 1) {
        const float tk = fwd_t_product<kPacked>(recs, raw, sorted, start, a, b, false, tx0, ty0, fpx, fpy, tid, s_r0, s_r1, s_r2, s_list);
        granule_store(gran_t, fs.epoch, tk);
      }
      const bool got = resolve_prefix(fs, rank, tid, k, fs.poll_budget, prefix);
      if (__syncthreads_or(got ? 0 : 1)) {  // (rare: the blocks in front have not run yet and may be waiting for this CU)
        if (tid == 0 && fs.fallbacks) atomicAdd(fs.fallbacks, 1);
        prefix = fwd_t_product<kPacked>(recs, raw, sorted, start, 0, a, true, tx0, ty0, fpx, fpy, tid, s_r0, s_r1, s_r2, s_list);
      }
    }
  }

  // Phase C: the forward's loop with T = prefix * (running product of the segment)
  const char *r0b = reinterpret_cast<const char *>(s_r0), *r1b = reinterpret_cast<const char *>(s_r1);
  const char *r2b = reinterpret_cast<const char *>(s_r2);
  const bool alive = inside && prefix >= kTMin;
  float tl = alive ? 1.0f : 0.0f, T = alive ? prefix : 0.0f, T_fin = -1.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, ad = 0.0f;
  [[maybe_unused]] float aq = 0.0f;  // (moment: Q, gs_render.h: DepthMaps)
  int n = -1;
  unsigned long long satmask = __ballot(!alive);
  int live = satmask != ~0ull ? 1 : 0;
  for (int base = a; base < b; base += kBatch) {
    const int count = min(kBatch, b - base);
    int t = tid;
    asm volatile("" : "+v"(t));
    __syncthreads();
    if (t < count) {
      const int g = sorted[start + base + t];
      SplatRec s = load_record<kPacked>(g, recs, raw);
      const unsigned int hits = block_hits(s, tx0, ty0);
      if (masks_out) masks_out[start + base + t] = (unsigned short)hits;
      stage_record(s);
      s.r1.w = __uint_as_float(hits);
      s.r2.w = s.r1.y > kLog2AlphaMax ? kLog2AlphaMax : s.r1.y;
      if constexpr (kDepth) s.r1.z = depth_value<kInv>(dm.xyz_c[3 * g + 2]);  // (gs_render.h: DepthMaps)
      s_r0[t] = s.r0; s_r1[t] = s.r1; s_r2[t] = s.r2;
    }
    __syncthreads();
    if (live > 0) {
      const int big = kBatch;
      unsigned short *lists = s_list + (t >> 6) * 4 * kListStride;
      const unsigned int list_lds =
          (unsigned int)(size_t)(__attribute__((address_space(3))) const unsigned short *)(lists + ((t >> 4) & 3) * kListStride);
      const RowCounts rc = build_row_lists<kListStride>(s_r1, lists, count, t >> 6, t & 63,
                                           (unsigned int)(satmask & 0xFFFFull) == 0xFFFFu ? 0 : big,
                                           (unsigned int)((satmask >> 16) & 0xFFFFull) == 0xFFFFu ? 0 : big,
                                           (unsigned int)((satmask >> 32) & 0xFFFFull) == 0xFFFFu ? 0 : big,
                                           (unsigned int)((satmask >> 48) & 0xFFFFull) == 0xFFFFu ? 0 : big, 2);
      const int trips = max(max(rc.c0, rc.c1), max(rc.c2, rc.c3));
      for (int i = 0; i < trips; i += 2) {
        int off0, off1;
        asm volatile("ds_read_u16 %0, %2\n\tds_read_u16 %1, %2 offset:2\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(off0), "=&v"(off1) : "v"(list_lds + 2 * i) : "memory");
        const float4 a0 = *reinterpret_cast<const float4 *>(r0b + off0), c0 = *reinterpret_cast<const float4 *>(r2b + off0);
        const float4 a1 = *reinterpret_cast<const float4 *>(r0b + off1), c1 = *reinterpret_cast<const float4 *>(r2b + off1);
        float2 b0, b1;
        float z0 = 0.0f, z1 = 0.0f;
        fwd_r1<kDepth>(r1b, off0, b0, z0);
        fwd_r1<kDepth>(r1b, off1, b1, z1);
        float al0 = staged_alpha_capped(a0.z, a0.w, b0.x, b0.y, c0.w, a0.x - fpx, a0.y - fpy);
        float al1 = staged_alpha_capped(a1.z, a1.w, b1.x, b1.y, c1.w, a1.x - fpx, a1.y - fpy);
        al0 = al0 > kAlphaMin ? al0 : 0.0f;
        al1 = al1 > kAlphaMin ? al1 : 0.0f;
        asm volatile("" : "+v"(al0), "+v"(al1));
        // (as in render_fwd_kernel: a saturated or dead pixel has tl = T = 0 and stays in the mask by itself)
        const float w0 = al0 * T;
        const float tl0 = __builtin_fmaf(-al0, tl, tl);
        const float tT0 = prefix * tl0;
        ar = __builtin_fmaf(c0.x, w0, ar);
        ag = __builtin_fmaf(c0.y, w0, ag);
        ab = __builtin_fmaf(c0.z, w0, ab);
        if constexpr (kDepth) ad = __builtin_fmaf(z0, w0, ad);
        if constexpr (kMom) aq = __builtin_fmaf(z0 * z0, w0, aq);
        const unsigned long long s0 = __ballot(tT0 < kTMin);
        tl = tl0;
        T = tT0;
        if (s0 != satmask) {
          if (((s0 & ~satmask) >> lane) & 1ull) { T_fin = tT0; n = base + (off0 >> 4) + 1; tl = 0.0f; T = 0.0f; }
          satmask = s0;
          if (satmask == ~0ull) { live = 0; i = trips; }
        }
        const float w1 = al1 * T;
        const float tl1 = __builtin_fmaf(-al1, tl, tl);
        const float tT1 = prefix * tl1;
        ar = __builtin_fmaf(c1.x, w1, ar);
        ag = __builtin_fmaf(c1.y, w1, ag);
        ab = __builtin_fmaf(c1.z, w1, ab);
        if constexpr (kDepth) ad = __builtin_fmaf(z1, w1, ad);
        if constexpr (kMom) aq = __builtin_fmaf(z1 * z1, w1, aq);
        const unsigned long long s1 = __ballot(tT1 < kTMin);
        tl = tl1;
        T = tT1;
        if (s1 != satmask) {
          if (((s1 & ~satmask) >> lane) & 1ull) { T_fin = tT1; n = base + (off1 >> 4) + 1; tl = 0.0f; T = 0.0f; }
          satmask = s1;
          if (satmask == ~0ull) {
            live = 0;
            break;
          }
        }
      }
    }
    if (__syncthreads_and(live <= 0 ? 1 : 0)) break;
  }
  // what the segment leaves behind: T in front of the next one (0 for a pixel that stopped or was dead: dead from here on)
  if (k < m - 1) granule_store(gran_f, fs.epoch, T);
  *part = make_float4(ar, ag, ab, T_fin >= 0.0f ? T_fin : T);
  if constexpr (kDepth) dm.part[(size_t)blk * 256 + tid] = ad;
  if constexpr (kMom) dm.part2[(size_t)blk * 256 + tid] = aq;
  *stop = T_fin >= 0.0f ? n : (alive ? -1 : -2);
}

#ifndef GS_FWD_WAVES
#define GS_FWD_WAVES 8
#endif
// kCompact: the forward also writes the compact lists for the backward (gs_render.h: CompactLists).  An instantiation of
// its own, for the scalar registers: the kernel sits at the 8-waves budget of both register files, and the compact form
// pays for its pointers and its running count with what the segment paths -- which it never runs beside -- hold.
template <bool kPacked, bool kDepth = false, bool kCompact = false, bool kInv = false, bool kMom = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GS_FWD_WAVES, 8))) void render_fwd_kernel(const float4 *__restrict__ recs, RawSplats raw,
                                                              const int *__restrict__ sorted,
                                                              const int *__restrict__ ranges, int width, int height,
                                                              int ntx, int num_tiles, float bg,
                                                              int *__restrict__ n_out, float *__restrict__ T_out,
                                                              float *__restrict__ image, float4 *__restrict__ zero,
                                                              long long zero_vec, unsigned short *__restrict__ masks_out,
                                                              const int *__restrict__ order, int *__restrict__ tops_out,
                                                              TileSegments seg, FwdSegments fs, DepthMaps dm,
                                                              CompactLists cl) {
  static_assert(kPacked || !kDepth, "depth mode is a mode of the context's (packed) kernels");
  static_assert(kPacked || !kCompact, "compact lists are written by the context's (packed) forward");
  static_assert(kDepth || (!kInv && !kMom), "inverse and moment are options of depth mode");
  __shared__ float4 s_r0[kBatch + 1], s_r1[kBatch + 1], s_r2[kBatch + 1];  // [kBatch]: the all-zero sentinel record
  __shared__ int s_tile_top;
  __shared__ int s_useful[4];  // compact lists (gs_render.h: CompactLists): the batch's useful slots, per staging wave
  __shared__ __attribute__((aligned(16))) unsigned short s_list[16 * kListStride + 2];
  // Optional side job: every workgroup clears its share of `zero` (the gradient rows the backward accumulates into).
  // This kernel leaves most of the HBM bandwidth unused, so the 64 bytes per gaussian ride along for free instead of
  // costing a memset between forward and backward.
  if (zero) {
    const long long per = (zero_vec + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = min(lo + per, zero_vec);
    for (long long k = lo + threadIdx.x; k < hi; k += 256) zero[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  // the segments of the long lists come first (gs_render.h: FwdSegments): each is a block of its own, and the tiles they
  // belong to have no block in the main grid
  // (the context's forward only: the stand-alone operator on the reference's arrays keeps one block per tile)
  const bool segmented = kPacked && !kCompact && fs.blocks != nullptr;
  if constexpr (kPacked && !kCompact) {
    if (segmented && (int)blockIdx.x < fs.cap) {
      if ((int)blockIdx.x < *fs.count)
        fwd_segment_block<kPacked, kDepth, kInv, kMom>(recs, raw, sorted, ranges, width, height, ntx, masks_out, fs, (int)blockIdx.x, s_r0, s_r1, s_r2, s_list, dm);
      return;
    }
  }
  const int tile = ordered_tile(order, segmented ? (int)blockIdx.x - fs.cap : (int)blockIdx.x, num_tiles);
  if (tile >= num_tiles) return;
  if (segmented && fs.rank[tile] >= 0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, row = lane >> 4, j = lane & 15;
#if GS_STAMP
  const unsigned long long st_t0 = GS_NOW(), st_rt0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long st_last = st_t0, st_bar = 0, st_bar1 = 0, st_bar2 = 0, st_stage = 0, st_lists = 0, st_loop = 0, st_trips = 0, st_batches = 0, st_load = 0;
#endif
  if (tid == 0) {
    s_r0[kBatch] = s_r2[kBatch] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s_r1[kBatch] = sentinel_r1();
    s_tile_top = 0;
  }
  const int tile_x = tile % ntx, tile_y = tile / ntx;
  const int px = tile_x * 16 + (wave & 1) * 8 + (row & 1) * 4 + (j & 3);
  const int py = tile_y * 16 + (wave >> 1) * 8 + (row >> 1) * 4 + (j >> 2);
  const bool inside = px < width && py < height;
  const float fpx = (float)px, fpy = (float)py;
  const float tx0 = (float)(tile_x * 16), ty0 = (float)(tile_y * 16);
  const char *r0b = reinterpret_cast<const char *>(s_r0), *r1b = reinterpret_cast<const char *>(s_r1);
  const char *r2b = reinterpret_cast<const char *>(s_r2);

  const int start = ranges[tile], total = ranges[tile + 1] - start;
  // A saturated pixel keeps T = 0 in the running transmittance, so every later splat blends with weight 0 and the
  // common path needs no per-pixel "done" masking; its real final transmittance and stop index live in T_fin / n.
  float T = inside ? 1.0f : 0.0f, T_fin = -1.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, ad = 0.0f;
  [[maybe_unused]] float aq = 0.0f;  // (moment: Q, gs_render.h: DepthMaps)
  int n = total;
  unsigned long long satmask = __ballot(!inside);  // lanes whose pixel is saturated or outside the image
  int live = satmask != ~0ull ? 1 : 0;
  // Compact lists (gs_render.h: CompactLists; the context's forward, one workgroup per tile): `cbase` counts the useful
  // entries of the batches so far (workgroup-uniform).  A pixel's stop index counted in useful entries is stored by the
  // batch that saturates it, behind the trip loop, and merged into the tile's maximum there: it is no register of the loop.
  constexpr bool compact = kCompact;
  int cbase = 0;

  static_assert(kSegEntries % kBatch == 0, "a segment boundary is a batch boundary of the forward");
  const bool checkpoints = !kCompact && seg.chk != nullptr && total > kSegSplitMin;  // a long list: the backward may walk it in segments
  for (int base = 0; base < total; base += kBatch) {
    const int count = min(kBatch, total - base);
    // an opaque per-batch copy of the thread index (see render_bwd_kernel): staging and list-building addresses are
    // rebuilt per batch instead of living in registers across the compositing loop
    int t = tid;
    asm volatile("" : "+v"(t));
    if (checkpoints && base > 0 && base % kSegEntries == 0) {  // (gs_render.h: TileSegments)
      seg.chk[(size_t)segment_slot(start, base / kSegEntries) * 256 + t] = make_float4(T, ar, ag, ab);
      if constexpr (kDepth) dm.chk[(size_t)segment_slot(start, base / kSegEntries) * 256 + t] = ad;
      if constexpr (kMom) dm.chk2[(size_t)segment_slot(start, base / kSegEntries) * 256 + t] = aq;
    }
#if GS_STAMP
    ++st_batches;
    GS_LAP(st_lists);  // (prologue of the first batch; nothing between the batches)
#endif
    __syncthreads();
    GS_LAP(st_bar);
    int g = 0;
    unsigned int hits = 0u;
    if (t < count) {
      g = sorted[start + base + t];
      SplatRec s = load_record<kPacked>(g, recs, raw);
#if GS_STAMP
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // split the staging stamp: loads | block test + LDS stores
      asm volatile("" : "+v"(s.r0.x), "+v"(s.r1.x), "+v"(s.r2.x));
      GS_LAP(st_load);
#endif
      hits = block_hits(s, tx0, ty0);
      if (masks_out) masks_out[start + base + t] = (unsigned short)hits;  // the backward stages the same instances
      stage_record(s);
      // The 0.99 cap goes into the exponent's own clamp (r04): alpha = exp2(min(q, log2 opa)) already has a per-gaussian
      // upper bound on q, so min(0.99, .) in the loop becomes the bound min(log2 opa, log2 0.99), formed here once per
      // (gaussian, tile).  It rides in r2.w, which the loop's 16-byte colour read fetches anyway; the block mask moves to
      // r1.w (the forward's loop reads only r1.xy).  A capped alpha comes out as exp2(kLog2AlphaMax), within two ulps
      // below 0.99f (the backward keeps its own 0.99f: it needs the uncapped value next to the capped one).  NaN stays NaN.
      s.r1.w = __uint_as_float(hits);
      s.r2.w = s.r1.y > kLog2AlphaMax ? kLog2AlphaMax : s.r1.y;
      if constexpr (kDepth) s.r1.z = depth_value<kInv>(dm.xyz_c[3 * g + 2]);  // (gs_render.h: DepthMaps; the loop never reads r1.z otherwise)
      s_r0[t] = s.r0; s_r1[t] = s.r1; s_r2[t] = s.r2;
    }
    unsigned int rank = 0u;  // of a useful slot among its staging wave's useful slots, inclusive
    if constexpr (kCompact) {
      // The rank rides in the high half of r1.w, above the 16 block bits (build_row_lists tests single bits): it is in
      // LDS before the barrier below, where the pixel that saturates on this slot -- a thread of any wave -- finds it.
      // (a 4-byte store of its own behind the record's: nothing of the record stays in registers for it)
      const unsigned long long useful = __ballot(hits != 0u);
      rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(useful >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)useful, 0u)) + 1u;
      if (hits != 0u) s_r1[t].w = __uint_as_float(hits | (rank << 16));
      if ((t & 63) == 0) s_useful[t >> 6] = __popcll(useful);
    }
    GS_LAP(st_stage);
    __syncthreads();
    GS_LAP(st_bar1);
    if constexpr (kCompact) {
      if (hits != 0u) {
        const int w = t >> 6;
        const size_t at = (size_t)start + cbase + (w > 0 ? s_useful[0] : 0) + (w > 1 ? s_useful[1] : 0) +
                          (w > 2 ? s_useful[2] : 0) + (rank - 1u);
        cl.ids[at] = g;
        cl.masks[at] = (unsigned short)hits;
      }
    }
    if (live > 0) {
      // rows whose 16 pixels are all saturated (or outside) need no list
      const int big = kBatch;
      unsigned short *lists = s_list + (t >> 6) * 4 * kListStride;
      const unsigned int list_lds =
          (unsigned int)(size_t)(__attribute__((address_space(3))) const unsigned short *)(lists + ((t >> 4) & 3) * kListStride);
      const RowCounts rc = build_row_lists<kListStride>(s_r1, lists, count, t >> 6, t & 63,
                                           (unsigned int)(satmask & 0xFFFFull) == 0xFFFFu ? 0 : big,
                                           (unsigned int)((satmask >> 16) & 0xFFFFull) == 0xFFFFu ? 0 : big,
                                           (unsigned int)((satmask >> 32) & 0xFFFFull) == 0xFFFFu ? 0 : big,
                                           (unsigned int)((satmask >> 48) & 0xFFFFull) == 0xFFFFu ? 0 : big, 2);
      const int trips = max(max(rc.c0, rc.c1), max(rc.c2, rc.c3));
#if GS_STAMP
      st_trips += (trips + 1) / 2;
      GS_LAP(st_lists);
#endif
      for (int i = 0; i < trips; i += 2) {
        // two list entries per trip: both records are fetched and both exponentials evaluated before the
        // (sequential) blending; a row past the end of its list reads the sentinel record and blends with alpha 0
        // (two zero-extending 16-bit reads: one 32-bit read costs an and and a shift on the VALU, which is what bounds
        // this loop; r04)
        int off0, off1;
        asm volatile("ds_read_u16 %0, %2\n\tds_read_u16 %1, %2 offset:2\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(off0), "=&v"(off1) : "v"(list_lds + 2 * i) : "memory");
        const float4 a0 = *reinterpret_cast<const float4 *>(r0b + off0), c0 = *reinterpret_cast<const float4 *>(r2b + off0);
        const float4 a1 = *reinterpret_cast<const float4 *>(r0b + off1), c1 = *reinterpret_cast<const float4 *>(r2b + off1);
        float2 b0, b1;
        float z0 = 0.0f, z1 = 0.0f;
        fwd_r1<kDepth>(r1b, off0, b0, z0);
        fwd_r1<kDepth>(r1b, off1, b1, z1);
        // (c.w: the exponent's bound, so the colour reads stay 16-byte reads -- a ds_read_b96 costs twice the LDS cycles)
        float al0 = staged_alpha_capped(a0.z, a0.w, b0.x, b0.y, c0.w, a0.x - fpx, a0.y - fpy);  // <= 0.99
        float al1 = staged_alpha_capped(a1.z, a1.w, b1.x, b1.y, c1.w, a1.x - fpx, a1.y - fpy);
        al0 = al0 > kAlphaMin ? al0 : 0.0f;
        al1 = al1 > kAlphaMin ? al1 : 0.0f;
        asm volatile("" : "+v"(al0), "+v"(al1));  // both evaluated (two independent chains) before the sequential blending
        // Invariant: T is either 0 (saturated or outside the image) or >= 1e-4, so "T (1 - alpha) < 1e-4" alone decides
        // whether a pixel is saturated behind this splat, and the compare's lane mask doubles as the saturation
        // bookkeeping.  A saturated pixel has T = 0, hence T (1 - alpha) = 0 < 1e-4: it stays in the mask by itself, and
        // the common path needs no select at all -- only the (rare) trip in which a pixel saturates zeroes its T (r04:
        // two v_cndmask fewer per trip; T (1 - alpha) as one FMA, T - alpha T).
        const float w0 = al0 * T;
        const float tT0 = __builtin_fmaf(-al0, T, T);
        ar = __builtin_fmaf(c0.x, w0, ar);
        ag = __builtin_fmaf(c0.y, w0, ag);
        ab = __builtin_fmaf(c0.z, w0, ab);
        if constexpr (kDepth) ad = __builtin_fmaf(z0, w0, ad);
        if constexpr (kMom) aq = __builtin_fmaf(z0 * z0, w0, aq);
        const unsigned long long s0 = __ballot(tT0 < kTMin);  // this splat was still accumulated (render.cu:76-87)
        T = tT0;
        if (s0 != satmask) {  // rare: some pixel saturated with the trip's first splat
          if (((s0 & ~satmask) >> lane) & 1ull) { T_fin = tT0; n = base + (off0 >> 4) + 1; T = 0.0f; }
          satmask = s0;
          // ... the wave's last live one: this trip is its last (the second splat blends with T = 0 everywhere, and the
          // test behind it finds nothing new: without this exit the wave walks the rest of the tile's list for nothing --
          // the dense scenes' forward took twice as long for a day of this round)
          if (satmask == ~0ull) { live = 0; i = trips; }
        }
        const float w1 = al1 * T;
        const float tT1 = __builtin_fmaf(-al1, T, T);
        ar = __builtin_fmaf(c1.x, w1, ar);
        ag = __builtin_fmaf(c1.y, w1, ag);
        ab = __builtin_fmaf(c1.z, w1, ab);
        if constexpr (kDepth) ad = __builtin_fmaf(z1, w1, ad);
        if constexpr (kMom) aq = __builtin_fmaf(z1 * z1, w1, aq);
        const unsigned long long s1 = __ballot(tT1 < kTMin);
        T = tT1;
        if (s1 != satmask) {  // rare: ... with its second
          if (((s1 & ~satmask) >> lane) & 1ull) { T_fin = tT1; n = base + (off1 >> 4) + 1; T = 0.0f; }
          satmask = s1;
          if (satmask == ~0ull) {
            live = 0;
            break;
          }
        }
      }
    }
    GS_LAP(st_loop);
    if constexpr (kCompact) {
      // Once per batch, behind the trip loop (which stays what it is: on the benchmark scene most pixels saturate, and the
      // trip that saturates one is not rare enough to carry this): a pixel that saturated in THIS batch -- on slot
      // n - 1 - base, an entry of a row list, hence useful -- stores its stop index counted in useful entries, the entry's
      // inclusive rank among the tile's useful ones.  The staged records and the staging waves' totals stand until the
      // next batch is staged, behind the barrier at the top of the loop.
      const int u0 = s_useful[0], u1 = s_useful[1], u2 = s_useful[2], u3 = s_useful[3];
      int n_c = 0;
      if (T_fin >= 0.0f && n > base) {
        const int sl = n - 1 - base, w = sl >> 6;
        n_c = cbase + (w > 0 ? u0 : 0) + (w > 1 ? u1 : 0) + (w > 2 ? u2 : 0) + (int)(__float_as_uint(s_r1[sl].w) >> 16);
        // (the pixel's position from the batch's opaque copy of the thread index: px and py stay out of the loop's registers)
        const int qx = tile_x * 16 + ((t >> 6) & 1) * 8 + ((t >> 4) & 1) * 4 + (t & 3);
        const int qy = tile_y * 16 + (t >> 7) * 8 + ((t >> 5) & 1) * 4 + ((t >> 2) & 3);
        cl.n_px[qy * width + qx] = n_c;
      }
      if (tops_out) {  // the tile's largest compact stop index (see below)
        const int m = row_max_int(n_c);
        const int wave_max = max(max(__builtin_amdgcn_readlane(m, 0), __builtin_amdgcn_readlane(m, 16)),
                                 max(__builtin_amdgcn_readlane(m, 32), __builtin_amdgcn_readlane(m, 48)));
        if ((t & 63) == 0 && wave_max > 0) atomicMax(&s_tile_top, wave_max);
      }
      cbase = __builtin_amdgcn_readfirstlane(cbase + u0 + u1 + u2 + u3);
    }
    const int all_done = __syncthreads_and(live <= 0 ? 1 : 0);
    GS_LAP(st_bar2);
    if (all_done) break;
  }
  // compact lists: a pixel that never saturated walks all of the tile's useful entries (its workgroup ranked every batch)
  const bool compact_all = compact && inside && !(T_fin >= 0.0f);
  if (tops_out) {
    // the tile's work in the backward = the largest stop index of its pixels (cuda/render_backward.cu:64,74): handed to
    // tile_order_kernel, which deals the backward's tiles heaviest first (counted in useful entries when the backward
    // walks the compact lists)
    int top = compact ? (compact_all ? cbase : 0) : inside ? n : 0;  // (compact: the saturated pixels have merged theirs)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = max(top, __shfl_xor(top, off, 64));
    if (lane == 0) atomicMax(&s_tile_top, top);
    __syncthreads();
    if (tid == 0) tops_out[tile] = s_tile_top;
  }
  if (inside) {
    const int pid = py * width + px;
    const float Tout = T_fin >= 0.0f ? T_fin : T;  // T_fin is set by the splat that saturated the pixel
    n_out[pid] = n;
    T_out[pid] = Tout;
    image[3 * pid + 0] = ar + Tout * bg;
    image[3 * pid + 1] = ag + Tout * bg;
    image[3 * pid + 2] = ab + Tout * bg;
    if constexpr (kDepth) dm.depth[pid] = ad;  // (background 0)
    if constexpr (kMom) dm.depth2[pid] = aq;
    if (compact_all) cl.n_px[pid] = cbase;
  }
  if (compact && tid == 0) cl.count[tile] = cbase;
#if GS_STAMP
  if (lane == 0) {
    unsigned long long *o = gs_stamp_fwd + ((size_t)blockIdx.x * 4 + wave) * GS_STAMP_WORDS;
    o[0] = (unsigned long long)tile; o[1] = st_rt0; o[2] = __builtin_amdgcn_s_memrealtime(); o[3] = GS_NOW() - st_t0;
    o[4] = st_bar; o[5] = st_stage; o[6] = st_lists; o[7] = st_loop; o[8] = st_load; o[9] = st_trips; o[10] = st_batches;
    o[11] = 0; o[12] = st_bar1; o[13] = st_bar2; o[14] = 0; o[15] = (unsigned long long)wave;
  }
#endif
}

// r05: the forward's segment blocks (gs_render.h: FwdSegments), by list length, in front of the forward.  The blocks are
// listed LAYER by layer -- all segments 0, then all segments 1, ... -- so that a segment starts when the segments in front
// of it are through wherever the layers fill the chip (no product pass then, and nothing at all for a segment nobody
// reaches), and side by side with them in the thin layers of the few longest lists.  With the long lists ranked by their
// number of segments m, longest first, layer k is the tiles of rank < L_k (L_k: lists with more than k segments): segment
// (t, k) is block base_k + rank_t, base_k = L_0 + ... + L_(k-1) -- one counting sort of the tiles by m in one workgroup's
// LDS.  A list of more than kFwdMaxLayers segments keeps its one block; if the blocks do not fit into the launch's room
// nothing is split (the next launch's room follows `asked`).
constexpr int kFwdMaxLayers = 128;
__global__ __launch_bounds__(1024) void fwd_segments_table_kernel(const int *__restrict__ ranges, int num_tiles, FwdSegments fs) {
  // [k]: lists of exactly k segments -> lists of more than k segments (suffix sums) | first block of layer k (prefix sums)
  __shared__ int s_more[kFwdMaxLayers + 2], s_base[kFwdMaxLayers + 2], s_cursor[kFwdMaxLayers + 2], s_tmp[kFwdMaxLayers + 2];
  const int tid = threadIdx.x;
  if (tid < kFwdMaxLayers + 2) s_more[tid] = s_cursor[tid] = 0;
  int m[kTableChunks];  // all of the thread's tiles up front (see tile_segments_kernel)
#pragma unroll
  for (int c = 0; c < kTableChunks; ++c) {
    const int t = c * 1024 + tid;
    m[c] = 0;
    if (t < num_tiles) {
      const int len = ranges[t + 1] - ranges[t];
      const int segs = len > kSegSplitMin ? (len + kSegEntries - 1) / kSegEntries : 0;
      m[c] = segs > kFwdMaxLayers ? 0 : segs;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kTableChunks; ++c)
    if (m[c] > 0) atomicAdd(&s_more[m[c]], 1);
  __syncthreads();
  // L_k = lists with more than k segments: exclusive suffix sums, then base_k = L_0 + .. + L_(k-1): exclusive prefix sums
  // (Hillis-Steele over 129 threads: a thread adding up its 128 predecessors one LDS read after the other took 7 us)
  const bool mine = tid <= kFwdMaxLayers;
  int v = mine ? s_more[tid] : 0;
  const int own = v;
  for (int off = 1; off <= kFwdMaxLayers; off <<= 1) {
    if (mine) s_tmp[tid] = v;
    __syncthreads();
    if (mine && tid + off <= kFwdMaxLayers) v += s_tmp[tid + off];
    __syncthreads();
  }
  const int more = v - own;
  if (mine) s_more[tid] = more;
  v = more;
  for (int off = 1; off <= kFwdMaxLayers; off <<= 1) {
    if (mine) s_tmp[tid] = v;
    __syncthreads();
    if (mine && tid >= off) v += s_tmp[tid - off];
    __syncthreads();
  }
  if (mine) {
    s_base[tid] = v - more;
    fs.base[tid] = v - more;
  }
  __syncthreads();
  const int total = s_base[kFwdMaxLayers];
  const bool fits = total <= fs.cap;
#pragma unroll
  for (int c = 0; c < kTableChunks; ++c) {
    const int t = c * 1024 + tid;
    if (t >= num_tiles) break;
    const int segs = fits ? m[c] : 0;
    int rank = -1;
    if (segs > 0) {
      rank = s_more[segs] + atomicAdd(&s_cursor[segs], 1);  // behind the lists of more segments
      for (int k = 0; k < segs; ++k) fs.blocks[s_base[k] + rank] = make_int2(t, k | (s_more[k] < fs.thin_layer ? 1 << 30 : 0));
    }
    fs.rank[t] = rank;
  }
  if (tid == 0) {
    *fs.count = fits ? total : 0;
    if (fs.asked) *fs.asked = tagged_figure(fs.tag, total);
  }
}

// ... and behind it: one block per tile adds up what the tile's segment blocks left (fixed order: the same image in every
// run), finds the segment the pixel stopped in and writes the forward's per-pixel outputs, the tile's largest stop index
// and the backward's checkpoints {T in front of the boundary, colour in front of it} (gs_render.h: TileSegments).
template <bool kDepth = false, bool kMom = false>
__global__ __launch_bounds__(256) void fwd_segments_combine_kernel(const int *__restrict__ ranges, int width, int height,
                                                                   int ntx, int num_tiles, float bg, int *__restrict__ n_out,
                                                                   float *__restrict__ T_out, float *__restrict__ image,
                                                                   int *__restrict__ tops_out, FwdSegments fs, TileSegments seg,
                                                                   DepthMaps dm) {
  __shared__ int s_top;
  const int tile = blockIdx.x;
  const int rank = fs.rank[tile];
  if (rank < 0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, row = lane >> 4, j = lane & 15;
  if (tid == 0) s_top = 0;
  __syncthreads();
  const int tile_x = tile % ntx, tile_y = tile / ntx;
  const int px = tile_x * 16 + (wave & 1) * 8 + (row & 1) * 4 + (j & 3);
  const int py = tile_y * 16 + (wave >> 1) * 8 + (row >> 1) * 4 + (j >> 2);
  const bool inside = px < width && py < height;
  const int start = ranges[tile], total = ranges[tile + 1] - start;
  const int m = (total + kSegEntries - 1) / kSegEntries;
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, ad = 0.0f, Tout = 1.0f;  // (depth: added in the colours' order)
  [[maybe_unused]] float aq = 0.0f;                               // (moment: Q likewise)
  int n = total;
  // kAhead segments' values are requested before the first is looked at: one at a time the longest list's twenty
  // segments were twenty dependent round trips (28 us behind the forward)
  constexpr int kAhead = 8;
  bool done = false;
  for (int k0 = 0; k0 < m && !done; k0 += kAhead) {
    int st[kAhead];
    float4 p[kAhead];
    float pref[kAhead], pd[kAhead];
    [[maybe_unused]] float pq[kAhead];
#pragma unroll
    for (int q = 0; q < kAhead; ++q) {
      const int k = min(k0 + q, m - 1);
      const size_t slot = (size_t)(fs.base[k] + rank);
      st[q] = fs.stop[slot * 256 + tid];
      p[q] = fs.part[slot * 256 + tid];
      pd[q] = kDepth ? dm.part[slot * 256 + tid] : 0.0f;
      if constexpr (kMom) pq[q] = dm.part2[slot * 256 + tid];
      // T in front of boundary k: what the segment in front left behind (read by the backward only for pixels that pass
      // the boundary alive, for which it is exactly the T segment k started from)
      pref[q] = k > 0 ? __uint_as_float((unsigned int)fs.granules[((size_t)fs.cap + fs.base[k - 1] + rank) * 256 + tid]) : 1.0f;
    }
#pragma unroll
    for (int q = 0; q < kAhead; ++q) {
      const int k = k0 + q;
      if (k >= m || done) break;
      if (k > 0 && seg.chk) {
        seg.chk[(size_t)segment_slot(start, k) * 256 + tid] = make_float4(pref[q], ar, ag, ab);
        if constexpr (kDepth) dm.chk[(size_t)segment_slot(start, k) * 256 + tid] = ad;
        if constexpr (kMom) dm.chk2[(size_t)segment_slot(start, k) * 256 + tid] = aq;
      }
      if (st[q] == -2) { done = true; break; }  // (a pixel outside the image; inside it a pixel is dead only behind the segment it stopped in)
      ar += p[q].x; ag += p[q].y; ab += p[q].z;
      if constexpr (kDepth) ad += pd[q];
      if constexpr (kMom) aq += pq[q];
      Tout = p[q].w;
      if (st[q] >= 0) { n = st[q]; done = true; }
    }
  }
  if (tops_out) {
    int top = inside ? n : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = max(top, __shfl_xor(top, off, 64));
    if (lane == 0) atomicMax(&s_top, top);
    __syncthreads();
    if (tid == 0) tops_out[tile] = s_top;
  }
  if (inside) {
    const int pid = py * width + px;
    n_out[pid] = n;
    T_out[pid] = Tout;
    image[3 * pid + 0] = ar + Tout * bg;
    image[3 * pid + 1] = ag + Tout * bg;
    image[3 * pid + 2] = ab + Tout * bg;
    if constexpr (kDepth) dm.depth[pid] = ad;
    if constexpr (kMom) dm.depth2[pid] = aq;
  }
}

int launch_fwd_segments_table(const int *ranges, int num_tiles, const FwdSegments &fs, hipStream_t st) {
  fwd_segments_table_kernel<<<1, 1024, 0, st>>>(ranges, num_tiles, fs);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int launch_render_fwd(const RenderFwdArgs &a, hipStream_t st) {
  const int ntx = (a.width + 15) / 16, nty = (a.height + 15) / 16, num_tiles = ntx * nty;
  const TileSegments &seg = a.segments;
  const FwdSegments &fs = a.fwd_segments;
  const bool packed = a.recs != nullptr, depth = a.depth.xyz_c != nullptr, compact = a.compact.ids != nullptr;
  GS_REQUIRE(!compact || (packed && !fs.blocks && !seg.chk), "compact lists: the context's unsegmented forward only");
  GS_REQUIRE(packed || !depth, "depth mode needs the packed records");
  const dim3 grid(tile_grid(num_tiles) + (fs.blocks ? fs.cap : 0));
  auto launch = [&](auto kernel) {  // (order: the forward takes its tiles as they come)
    launch_tiles(kernel, grid, st, nullptr, nullptr, a.recs, a.raw, a.sorted, a.ranges, a.width, a.height, ntx, num_tiles, a.bg,
                 a.n_out, a.T_out, a.image, a.zero, a.zero_vec, a.masks_out, nullptr, a.tops_out, seg, fs, a.depth, a.compact);
  };
  const bool inv = depth && a.depth.inverse, mom = depth && a.depth.moment;  // (gs_render.h: DepthMaps, the options)
  GS_REQUIRE(!mom || a.depth.depth2, "the moment option needs its map");
  if (inv || mom) {  // the options' own instantiations; the ones below are what they were
    if (compact) {
      if (inv && mom) launch(render_fwd_kernel<true, true, true, true, true>);
      else if (mom) launch(render_fwd_kernel<true, true, true, false, true>);
      else launch(render_fwd_kernel<true, true, true, true, false>);
    } else {
      if (inv && mom) launch(render_fwd_kernel<true, true, false, true, true>);
      else if (mom) launch(render_fwd_kernel<true, true, false, false, true>);
      else launch(render_fwd_kernel<true, true, false, true, false>);
    }
  }
  else if (compact) depth ? launch(render_fwd_kernel<true, true, true>) : launch(render_fwd_kernel<true, false, true>);
  else if (packed) depth ? launch(render_fwd_kernel<true, true>) : launch(render_fwd_kernel<true>);
  else launch(render_fwd_kernel<false>);
  GS_LAUNCH_CHECK();
  if (fs.blocks) {
    auto combine = [&](auto kernel) {
      kernel<<<num_tiles, 256, 0, st>>>(a.ranges, a.width, a.height, ntx, num_tiles, a.bg, a.n_out, a.T_out, a.image, a.tops_out, fs, seg, a.depth);
    };
    if (mom) combine(fwd_segments_combine_kernel<true, true>);
    else depth ? combine(fwd_segments_combine_kernel<true>) : combine(fwd_segments_combine_kernel<false>);
    GS_LAUNCH_CHECK();
  }
  return GSPLAT_OK;
}

}  // namespace gs

extern "C" {

#if GS_STAMP
// diagnostic builds only: copies the stamp words of the last render_fwd launch (GS_STAMP_WORDS per wave, 4 waves per block)
int gsplat_debug_read_stamps_fwd(unsigned long long *dst, size_t words) {
  (void)hipDeviceSynchronize();
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(gs_stamp_fwd), words * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif

int gsplat_render_image(const float *uv, const float *opacity, const float *conic, const float *rgb,
                        float background_opacity, const int *sorted_splats, const int *splat_range_by_tile,
                        int image_width, int image_height, int *splats_per_pixel, float *weight_per_pixel,
                        float *image, void *stream) {
  GS_REQUIRE_DEV(uv); GS_REQUIRE_DEV(opacity); GS_REQUIRE_DEV(conic); GS_REQUIRE_DEV(rgb);
  GS_REQUIRE_DEV(sorted_splats); GS_REQUIRE_DEV(splat_range_by_tile); GS_REQUIRE_DEV(splats_per_pixel);
  GS_REQUIRE_DEV(weight_per_pixel); GS_REQUIRE_DEV(image);
  GS_REQUIRE(image_width > 0 && image_height > 0, "image size must be positive");
  gs::RenderFwdArgs a = {};
  a.raw.uv = uv; a.raw.opacity = opacity; a.raw.conic = conic; a.raw.rgb = rgb;
  a.sorted = sorted_splats; a.ranges = splat_range_by_tile;
  a.width = image_width; a.height = image_height; a.bg = background_opacity;
  a.n_out = splats_per_pixel; a.T_out = weight_per_pixel; a.image = image;
  return gs::launch_render_fwd(a, (hipStream_t)stream);
}

}  // extern "C"
